"""The float32 LayerNorm as one launch on the MI355X (layernorm_f32_kernel,
BAND_HIP_FUSED_LAYERNORM_F32=1), held to the numpy restatement of
tests.layernorm_f32_models bit for bit: the launcher on every case, data kind
and alignment with the output alone, the quantised rows alone (both forms) and
both; the patterns around every output; a row alone against the same row
among nine; the refusals; then the models through the kGPU executor - launch
counts, outputs exact against the rule over an eager pass, the capture and a
replay, the encoder blocks op by op when every tensor is viewed and exact at
the projections that read the two LayerNorms otherwise, job batches, and the
switches that turn the fused launch off.

The encoder blocks' final output is not replayed on the host: the float
BATCH_MATMUL, SOFTMAX and GELU between the norms go through the device's expf /
erff and its own summation order, which numpy does not reproduce bit for bit.
Instead the first block's Q, K and V projections (extra model outputs of
encoder_with_qkv_outputs) and the MLP's first projection - every op that reads
a fused LayerNorm - must equal the rule applied to the run's own LayerNorm
input, bit for bit."""
import ctypes

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
from oracle.tflite_fb import Model as OModel
from tests import float_harness as H
from tests import hybrid_models as Y
from tests import layernorm_f32_models as L

pytestmark = pytest.mark.gpu

F = np.float32
_REFS = {}


def _ref(case):
    """the restated y of a case and its quantised rows in both forms, computed once"""
    if case.name not in _REFS:
        y = case.ref()
        _REFS[case.name] = (y, Y.np_dynquant(y, False), Y.np_dynquant(y, True))
    return _REFS[case.name]


def _assert_launch(case, lib, mode, off):
    y, q, s, o = L.launch(case, lib, mode, off)
    ry, sym, asym = _ref(case)
    what = "%s %s off %d" % (case.name, mode, off)
    if y is not None:
        np.testing.assert_array_equal(y.view(np.uint32), ry.view(np.uint32), err_msg=what + " y")
    if q is not None:
        rq, rs, ro = asym if mode.endswith("asym") else sym
        np.testing.assert_array_equal(q, rq, err_msg=what + " q")
        np.testing.assert_array_equal(s.view(np.uint32), rs.view(np.uint32), err_msg=what + " scale")
        np.testing.assert_array_equal(o, ro, err_msg=what + " offset")


@pytest.mark.parametrize("off", [0, 4])
@pytest.mark.parametrize("shape", L.SHAPES, ids=lambda s: "%dx%d" % s)
def test_launcher(gpu_lib, shape, off):
    """every data kind and mode of one shape and alignment"""
    for kind in L.KINDS:
        case = L.LnCase(*shape, kind)
        for mode in L.MODES:
            _assert_launch(case, gpu_lib, mode, off)


@pytest.mark.parametrize("off", [0, 4])
def test_launcher_nonfinite(gpu_lib, off):
    """+-inf and NaN at known positions, output only: NaN exactly where the restatement has it, the rest equal"""
    case = L.LnCase(*L.NONFINITE_SHAPE, "nonfinite")
    y, _, _, _ = L.launch(case, gpu_lib, "out", off)
    ref = case.ref()
    assert np.isnan(ref[1:4]).all() and np.isfinite(ref[0]).all() and np.isfinite(ref[4]).all()
    np.testing.assert_array_equal(np.isnan(y), np.isnan(ref))
    keep = ~np.isnan(ref)
    np.testing.assert_array_equal(y[keep].view(np.uint32), ref[keep].view(np.uint32))


@pytest.mark.parametrize("shape", [(9, 1023), (9, 192)], ids=lambda s: "%dx%d" % s)
def test_a_row_alone_equals_the_row_among_nine(gpu_lib, shape):
    """rows 1 and 8 of nine (the second wave of a workgroup; a partial workgroup) as the only row of a launch"""
    case = L.LnCase(*shape, "normal")
    y9, q9, s9, o9 = L.launch(case, gpu_lib, "both_asym")
    for row in (1, 8):
        one = L.LnCase(1, shape[1], "normal")
        one.x, one.gamma, one.beta = case.x[row:row + 1].copy(), case.gamma, case.beta
        for off in (0, 4):
            y1, q1, s1, o1 = L.launch(one, gpu_lib, "both_asym", off)
            np.testing.assert_array_equal(y1[0].view(np.uint32), y9[row].view(np.uint32))
            np.testing.assert_array_equal(q1[0], q9[row])
            assert s1[0].tobytes() == s9[row].tobytes() and o1[0] == o9[row]


def test_launcher_refuses_bad_parameters(gpu_lib):
    """non-zero, the reason named, and nothing launched: the outputs keep their fill"""
    from band_amd.device import DeviceBuffer
    fill = Y._filled(4096, L.NAN_WORD)
    buf = DeviceBuffer.from_array(fill)
    for name, change, reason in L.REFUSALS:
        p = L.valid_block(buf.value)
        assert gpu_lib.bh_layernorm_f32_kernel(ctypes.byref(p)) == L.KERNEL.encode(), gpu_lib.bh_last_error()
        for k, v in change.items():
            setattr(p, k, v)
        assert gpu_lib.bh_layernorm_f32_kernel(ctypes.byref(p)) == b"", name
        assert gpu_lib.bh_layernorm_f32(ctypes.byref(p), None) != 0, name
        msg = gpu_lib.bh_last_error().decode()
        assert msg.startswith("bh_layernorm_f32: ") and reason in msg, msg
    assert gpu_lib.bh_layernorm_f32(None, None) != 0
    assert (buf.download(np.uint8, (4096,)) == fill).all()


# ---- models ------------------------------------------------------------------------------
def _exec(buf, mid=0, flag=DeviceFlag.kGPU, worker=1):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(mid, worker, flag)
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    ex._model_ref = m
    return m, ex, SubgraphKey(mid, worker)


def _run(buf, feeds, view, flag=DeviceFlag.kGPU, worker=1):
    """tests.float_harness.run_executor that also hands back the launch list after the views were taken.
    view: "all", "outputs" or a list of extra tensors beside the outputs"""
    om = OModel(buf)
    m, ex, key = _exec(buf, 0, flag, worker)
    if view == "all":
        want = sorted({t for o in om.operators for t in o.outputs})
    else:
        want = list(om.outputs) + ([] if view == "outputs" else list(view))
    views = {t: ex.GetTensorView(key, t) for t in want}
    runs = []
    for feed in feeds:
        for t in om.inputs:
            ex.GetTensorView(key, t).GetData()[...] = feed[t]
        assert ex.ExecuteSubgraph(key).ok()
        vals = {t: v.GetData().copy() for t, v in views.items()}
        for t in om.inputs:
            vals[t] = np.asarray(feed[t], F)
        runs.append(vals)
    return om, ex.LaunchKernels(key), runs


@pytest.fixture
def flag_on(monkeypatch):
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    monkeypatch.setenv(L.FLAG, "1")


def _counts(kernels):
    return {k: kernels.count(k) for k in (L.KERNEL, Y.DQ_KERNEL, Y.FC_KERNEL) + L.OP_KERNELS}


def test_ln_only_is_one_launch_and_exact(gpu_lib, flag_on):
    buf = L.ln_only()
    feeds = [Y.model_feed(buf, seed=50 + i) for i in range(3)]
    om, kernels, runs = _run(buf, feeds, "outputs")
    assert kernels == [L.KERNEL], kernels
    (ln,) = L.layer_norms(om)
    for i, vals in enumerate(runs):  # eager, capture, replay
        ref = L.model_layernorm(om, ln, vals[ln[0]])
        np.testing.assert_array_equal(vals[ln[4]].reshape(ref.shape).view(np.uint32), ref.view(np.uint32),
                                      err_msg="run %d" % i)


@pytest.mark.parametrize("which", sorted(L.LN_OP_OF))
def test_an_intermediate_that_is_a_model_output_keeps_the_ten_launches(gpu_lib, flag_on, monkeypatch, which):
    """a LayerNorm whose row mean m, or whose a = x * g, is a model output beside y: the fused launch
    would not store it, so with the flag on the ten ops stay ten launches, and every output is the
    bytes of the run with BAND_HIP_FUSION=nolayernorm"""
    buf = L.ln_with_intermediate_output(which)
    feeds = [Y.model_feed(buf, seed=60 + i) for i in range(2)]
    om, kernels, runs = _run(buf, feeds, "outputs")
    assert len(om.outputs) == 2
    assert len(kernels) == 10 and L.KERNEL not in kernels, kernels
    assert (kernels.count("mean_kernel"), kernels.count("unary_f32_kernel"), kernels.count("eltwise_f32_kernel")) == \
        (2, 1, 7), kernels
    monkeypatch.setenv("BAND_HIP_FUSION", "nolayernorm")
    _, kernels_off, runs_off = _run(buf, feeds, "outputs")
    assert kernels == kernels_off
    for vals, ref in zip(runs, runs_off):
        for t in om.outputs:
            assert vals[t].tobytes() == ref[t].tobytes(), "tensor %d" % t


@pytest.mark.parametrize("name", ["ln_qkv_symmetric", "ln_qkv_asymmetric", "ln_mixed"])
def test_projections_of_a_fused_layernorm_are_exact(gpu_lib, flag_on, name):
    """every FULLY_CONNECTED equals np_fc_from_q(np_dynquant(np_layernorm_f32(x))) bit for bit; ln_qkv: one LayerNorm
    launch, no quantisation launch, three products; ln_mixed: the asymmetric reader keeps its launch (and y is stored)"""
    buf = L.MODELS[name]()
    feeds = [Y.model_feed(buf, seed=60 + i) for i in range(3)]
    om, kernels, runs = _run(buf, feeds, "outputs")
    n = _counts(kernels)
    if name == "ln_mixed":
        assert n[L.KERNEL] == 1 and n[Y.DQ_KERNEL] == 1 and n[Y.FC_KERNEL] == 2 and len(kernels) == 4, kernels
    else:
        assert n[L.KERNEL] == 1 and n[Y.DQ_KERNEL] == 0 and n[Y.FC_KERNEL] == 3 and len(kernels) == 4, kernels
    assert not any(n[k] for k in L.OP_KERNELS), kernels
    (ln,) = L.layer_norms(om)
    fcs = [o for o in om.operators if Y.is_hybrid_fc(om, o)]
    assert len(fcs) == (2 if name == "ln_mixed" else 3) and all(o.inputs[0] == ln[4] for o in fcs)
    for i, vals in enumerate(runs):
        y = L.model_layernorm(om, ln, vals[ln[0]])
        for o in fcs:
            ref = L.fc_from_rows(om, o, y)
            np.testing.assert_array_equal(vals[o.outputs[0]].reshape(ref.shape).view(np.uint32), ref.view(np.uint32),
                                          err_msg="%s run %d op output %d" % (name, i, o.outputs[0]))


def test_ln_fc_and_add_folds_the_quantisation_and_still_stores_y(gpu_lib, flag_on):
    buf = L.ln_fc_and_add()
    feeds = [Y.model_feed(buf, seed=70 + i) for i in range(3)]
    om, kernels, runs = _run(buf, feeds, "outputs")
    n = _counts(kernels)
    assert n[L.KERNEL] == 1 and n[Y.DQ_KERNEL] == 0 and n[Y.FC_KERNEL] == 1, kernels
    assert kernels.count("eltwise_f32_kernel") == 1 and len(kernels) == 3, kernels  # the ADD that reads y
    (ln,) = L.layer_norms(om)
    (fc,) = [o for o in om.operators if Y.is_hybrid_fc(om, o)]
    (add,) = [o for o in om.operators if o.name == "ADD" and ln[4] in o.inputs and ln[0] in o.inputs]
    for i, vals in enumerate(runs):
        x = np.asarray(vals[ln[0]], F)
        y = L.model_layernorm(om, ln, x)
        ref = L.fc_from_rows(om, fc, y)
        np.testing.assert_array_equal(vals[fc.outputs[0]].reshape(ref.shape).view(np.uint32), ref.view(np.uint32))
        s = (y + x.reshape(y.shape)).astype(F)  # the stored y, through one float32 addition
        np.testing.assert_array_equal(vals[add.outputs[0]].reshape(s.shape).view(np.uint32), s.view(np.uint32))


@pytest.mark.parametrize("name", L.ENCODERS)
def test_encoder_block_every_tensor_viewed_is_op_by_op(gpu_lib, flag_on, name):
    """a view of every tensor re-lowers the LayerNorms op by op: the ten launches are back, six quantisation launches,
    and every op passes its own check"""
    buf = Y.MODELS[name]()
    feeds = [Y.model_feed(buf, seed=30 + i) for i in range(2)]
    om, kernels, runs = _run(buf, feeds, "all")
    n = _counts(kernels)
    assert n[L.KERNEL] == 0 and n["mean_kernel"] == 4 and n["unary_f32_kernel"] >= 2 and n[Y.DQ_KERNEL] == 6, kernels
    for i, vals in enumerate(runs):
        assert H.check_graph_ops(om, vals, "%s run %d" % (name, i), gelu_ulps=16)[1]["fc"] == 6


@pytest.mark.parametrize("form", ["symmetric", "asymmetric"])
def test_encoder_block_fused_is_20_launches_and_exact_at_the_projections(gpu_lib, flag_on, form):
    """see the module docstring: Q, K, V and the MLP's first projection against the rule on the run's own inputs"""
    buf = L.encoder_with_qkv_outputs(form)
    om = OModel(buf)
    lns = L.layer_norms(om)
    assert len(lns) == 2
    fcs = [o for o in om.operators if Y.is_hybrid_fc(om, o)]
    readers = [[o for o in fcs if o.inputs[0] == ln[4]] for ln in lns]
    assert [len(r) for r in readers] == [3, 1]
    assert set(om.outputs[1:]) == {o.outputs[0] for o in readers[0]}
    # the second LayerNorm's input and the MLP's first projection are read by later ops: viewing them de-fuses nothing
    extra = [lns[1][0], readers[1][0].outputs[0]]
    feeds = [Y.model_feed(buf, seed=80 + i) for i in range(3)]
    om, kernels, runs = _run(buf, feeds, extra)
    n = _counts(kernels)
    assert len(kernels) == 20 and n[L.KERNEL] == 2 and n[Y.DQ_KERNEL] == 2 and n[Y.FC_KERNEL] == 6, kernels
    assert not any(n[k] for k in ("mean_kernel",)), kernels
    for i, vals in enumerate(runs):
        for ln, rd in zip(lns, readers):
            y = L.model_layernorm(om, ln, vals[ln[0]])
            for o in rd:
                ref = L.fc_from_rows(om, o, y)
                np.testing.assert_array_equal(vals[o.outputs[0]].reshape(ref.shape).view(np.uint32),
                                              ref.view(np.uint32), err_msg="%s run %d" % (form, i))
        assert np.isfinite(vals[om.outputs[0]]).all()


def test_encoder_block_outputs_only_has_20_launches(gpu_lib, flag_on):
    buf = Y.MODELS[L.ENCODERS[1]]()
    om, kernels, runs = _run(buf, [Y.model_feed(buf, seed=1)], "outputs")
    assert len(kernels) == 20 and kernels.count(L.KERNEL) == 2 and kernels.count(Y.DQ_KERNEL) == 2, kernels
    assert np.isfinite(runs[0][om.outputs[0]]).all()


def test_job_batches(gpu_lib, flag_on):
    """jobs of a batch of 2, 3 and 5 equal their own single-job runs; a variant launches its parent's kernels"""
    buf = L.ln_qkv("asymmetric")
    feeds = [Y.model_feed(buf, seed=40 + s) for s in range(5)]
    om, kernels, singles = _run(buf, feeds, "outputs")
    assert kernels.count(L.KERNEL) == 1 and kernels.count(Y.DQ_KERNEL) == 0
    m, ex, key = _exec(buf, 91)
    st = ex.PrepareJobBatches(m, key, 5)
    assert st.ok(), st.message()
    assert ex.MaxJobBatch(key) == 5
    t_in = ex.GetInputs(key)[0]
    for n in (2, 3, 5):
        assert ex.JobBatchLaunchKernels(key, n) == kernels
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


@pytest.mark.parametrize("env,flag", [({}, DeviceFlag.kGPU), ({L.FLAG: "0"}, DeviceFlag.kGPU),
                                      ({L.FLAG: "1", "BAND_HIP_FUSION": "nolayernorm"}, DeviceFlag.kGPU),
                                      ({L.FLAG: "1", "BAND_HIP_FUSION": "0"}, DeviceFlag.kGPU),
                                      ({L.FLAG: "1"}, DeviceFlag.kCPU)],
                         ids=["unset", "zero", "nolayernorm", "fusion_0", "kcpu"])
def test_switches_keep_the_ten_launches(gpu_lib, monkeypatch, env, flag):
    monkeypatch.delenv(L.FLAG, raising=False)
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    buf = L.ln_qkv("symmetric")
    m, ex, key = _exec(buf, 0, flag, 1 if flag == DeviceFlag.kGPU else 0)
    kernels = ex.LaunchKernels(key)
    assert not any("layernorm_f32" in k for k in kernels), kernels
    assert len(kernels) == 16, kernels
    if flag == DeviceFlag.kGPU:
        assert kernels.count("mean_kernel") == 2 and kernels.count(Y.DQ_KERNEL) == 3, kernels
