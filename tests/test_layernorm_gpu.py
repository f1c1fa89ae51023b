"""The LayerNorm / GELU ops on the MI355X: mean_rows_kernel and
eltwise_sqdiff_kernel on the cases of tests.encoder_models (kernel name first,
0xff past the output must stay), the RSQRT and 8-bit GELU tables through
bh_lut_u8 on all 256 codes, float GELU through bh_unary_f32, bh_layernorm_i8
against the numpy chain of the ten ops (and what it refuses), and the models
through the kGPU executor (eager then replayed twice, outputs only - one
layernorm_i8_kernel launch per LayerNorm - and every tensor viewed - nothing
fused; BAND_HIP_FUSION=nolayernorm; job batches 2, 3, 5) and a GPU-only engine.

References: the numpy restatements of tests.encoder_models (held against the
real-valued functions in tests/test_layernorm_cpu.py) and run_reference;
every int8 / uint8 tensor is compared with assert_array_equal."""
import ctypes

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi
from oracle.tflite_fb import Model as OModel
from tests import encoder_models as E
from tests.graph_reference import run_reference

pytestmark = pytest.mark.gpu

MEAN_CASES = E.mean_cases()
SQDIFF_CASES = E.sqdiff_cases()
F = np.float32


@pytest.mark.parametrize("case", MEAN_CASES, ids=lambda c: c.name)
def test_mean_rows_launcher(gpu_lib, case):
    np.testing.assert_array_equal(E.launch_mean(case, gpu_lib, True), case.ref(), err_msg=case.name)


def test_mean_rows_refuses_bad_parameters(gpu_lib):
    from band_amd.device import DeviceBuffer
    bufs = [DeviceBuffer(256) for _ in range(2)]
    for name, kw, reason in (("null_out", dict(output=None), "null pointer"), ("zero_rows", dict(rows=0), "non-positive"),
                             ("negative_depth", dict(depth=-1), "non-positive"), ("type", dict(type=3), "type must be"),
                             ("row_sum", dict(depth=1 << 24), "depth * 255 >= 2^31")):
        p = _abi.MeanRowsParams()
        p.rows, p.depth, p.type, p.exact, p.input, p.output = 2, 8, 1, 1, bufs[0].value, bufs[1].value
        assert gpu_lib.bh_mean_rows_kernel(ctypes.byref(p)) == E.MEAN_KERNEL.encode()
        for k, v in kw.items():
            setattr(p, k, v)
        assert gpu_lib.bh_mean_rows_kernel(ctypes.byref(p)) == b"", name
        assert gpu_lib.bh_mean_rows(ctypes.byref(p), None) != 0
        msg = gpu_lib.bh_last_error().decode()
        assert msg.startswith("bh_mean_rows: ") and reason in msg, msg
    assert gpu_lib.bh_mean_rows(None, None) != 0


@pytest.mark.parametrize("case", SQDIFF_CASES, ids=lambda c: c.name)
def test_sqdiff_launcher(gpu_lib, case):
    np.testing.assert_array_equal(E.launch_sqdiff(case, gpu_lib, True), case.ref(), err_msg=case.name)


def test_sqdiff_refuses_bad_parameters(gpu_lib):
    from band_amd.device import DeviceBuffer
    bufs = [DeviceBuffer(256) for _ in range(3)]
    case = SQDIFF_CASES[0]
    for name, change, reason in (("uint8", lambda p: setattr(p, "in_signed", 0), "int8 only"),
                                 ("null", lambda p: setattr(p, "b", None), "null pointer"),
                                 ("shift", lambda p: setattr(p, "o_shift", 1), "shifts out of range"),
                                 ("broadcast", lambda p: p.shape_b.__setitem__(3, 2), "bad shape")):
        p = E.eltwise_params(case, *(b.value for b in bufs))
        change(p)
        assert gpu_lib.bh_eltwise_i8(ctypes.byref(p), None) != 0, name
        msg = gpu_lib.bh_last_error().decode()
        assert msg.startswith("bh_eltwise_i8: ") and reason in msg, msg


def _lut(gpu_lib, table):
    from band_amd.device import DeviceBuffer
    codes = np.arange(256, dtype=np.uint8)
    dx, dt = DeviceBuffer.from_array(codes), DeviceBuffer.from_array(table)
    dy = DeviceBuffer.from_array(np.full(256 + 16, 0xff, np.uint8))
    _abi.check(gpu_lib.bh_lut_u8(dx.value, dy.value, 256, dt.value, None), "bh_lut_u8")
    got = dy.download(np.uint8, (256 + 16,))
    assert (got[256:] == 0xff).all()
    return got[:256]


def test_rsqrt_and_gelu_tables_through_the_lut_kernel(gpu_lib):
    """the library's tables (what the executor uploads) gathered on the device for all 256 codes"""
    t = np.zeros(256, np.uint8)
    for q in E.RSQRT_Q:
        assert gpu_lib.bhx_rsqrt_table(q[0], q[1], q[2], q[3], t.ctypes.data) == 0
        np.testing.assert_array_equal(_lut(gpu_lib, t), E.np_rsqrt_table(*q))
    for signed, s_in, z_in, s_out, z_out in E.GELU_Q:
        for approx in (0, 1):
            assert gpu_lib.bhx_gelu_table(int(signed), approx, s_in, z_in, s_out, z_out, t.ctypes.data) == 0
            np.testing.assert_array_equal(_lut(gpu_lib, t), E.np_gelu_table(signed, bool(approx), s_in, z_in, s_out, z_out))


def test_float_gelu(gpu_lib):
    """bh_unary_f32 GELU against float64 at E.gelu_f32_bound with 16 ulp for the
    device erff / tanhf.  No ULP table of the device library is installed with
    ROCm here; 16 is what OpenCL's full profile allows erf (5 for tanh), the
    profile the device library's math functions are written to."""
    from band_amd.device import DeviceBuffer
    x = np.concatenate([np.linspace(-10, 10, 4001), [0.0, 1e-30, -1e-30, 1e-20, -1e-20, 10.0, -10.0]]).astype(F)
    dx, dy = DeviceBuffer.from_array(x), DeviceBuffer.from_array(np.zeros_like(x))
    for kind, approx in ((3, False), (4, True)):
        _abi.check(gpu_lib.bh_unary_f32(kind, dx.value, dy.value, x.size, 0.0, 0.0, None), "bh_unary_f32")
        y = dy.download(np.float32, x.shape)
        ref = np.array([E.gelu_real(float(v), approx) for v in x])
        err, tol = np.abs(y.astype(np.float64) - ref), E.gelu_f32_bound(x, ref, 16)
        print("gelu approx=%d worst err / tol %.3g" % (approx, (err / tol).max()))
        assert (err <= tol).all(), (x[err > tol][:5], err[err > tol][:5])
    assert gpu_lib.bh_unary_f32(5, dx.value, dy.value, x.size, 0.0, 0.0, None) != 0


# ---- the fused launch ----------------------------------------------------------------------
LN_CASES = E.ln_cases()


@pytest.mark.parametrize("case", LN_CASES, ids=lambda c: c.name)
def test_layernorm_launcher(gpu_lib, case):
    """bh_layernorm_i8 against the numpy chain of the ten ops"""
    np.testing.assert_array_equal(E.launch_ln(case, gpu_lib), case.ref(), err_msg=case.name)


def test_layernorm_refuses_a_row_above_the_limit(gpu_lib):
    case = E.LnCase(3, 4100)
    p, keep = E.launch_ln(case, gpu_lib, check_only=True)
    assert gpu_lib.bh_layernorm_i8_kernel(ctypes.byref(p)) == b""
    assert gpu_lib.bh_layernorm_i8(ctypes.byref(p), None) != 0
    assert "depth above 1024" in gpu_lib.bh_last_error().decode()


LN_REFUSED = [("null_gamma", lambda p: setattr(p, "gamma", None), "null pointer"),
              ("null_table", lambda p: setattr(p, "rsqrt_table", None), "null pointer"),
              ("zero_rows", lambda p: setattr(p, "rows", 0), "non-positive"),
              ("depth_limit", lambda p: setattr(p, "depth", 1025), "depth above 1024"),
              ("mean_depth", lambda p: setattr(p.mean_d, "depth", 7), "MEAN blocks"),
              ("uint8_mean", lambda p: setattr(p.mean_x, "type", 2), "MEAN blocks"),
              ("sqdiff_kind", lambda p: setattr(p.sqdiff, "kind", 0), "SQUARED_DIFFERENCE block"),
              ("add_kind", lambda p: setattr(p.add_eps, "kind", 1), "ADD / SUB block"),
              ("add_shift", lambda p: setattr(p.add_out, "o_shift", 1), "ADD / SUB block"),
              ("mul_unsigned", lambda p: setattr(p.mul_x, "in_signed", 0), "MUL block"),
              ("eps_range", lambda p: setattr(p, "eps_q", 200), "eps_q")]


@pytest.mark.parametrize("name,change,reason", LN_REFUSED, ids=[r[0] for r in LN_REFUSED])
def test_layernorm_refuses_bad_parameters(gpu_lib, name, change, reason):
    p, keep = E.launch_ln(LN_CASES[2], gpu_lib, check_only=True)
    assert gpu_lib.bh_layernorm_i8_kernel(ctypes.byref(p)) == E.LN_KERNEL.encode()
    change(p)
    assert gpu_lib.bh_layernorm_i8_kernel(ctypes.byref(p)) == b""
    assert gpu_lib.bh_layernorm_i8(ctypes.byref(p), None) != 0
    msg = gpu_lib.bh_last_error().decode()
    assert msg.startswith("bh_layernorm_i8: ") and reason in msg, msg
    assert gpu_lib.bh_layernorm_i8(None, None) != 0


# ---- models ------------------------------------------------------------------------------
def _exec(buf, mid):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(mid, 1, DeviceFlag.kGPU)
    spec = ex.InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kGPU] == set(), spec.unsupported_ops  # registers whole on the GPU
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    ex._model_ref = m
    return m, ex, SubgraphKey(mid, 1)


@pytest.fixture(scope="module")
def model_refs():
    out = {}
    for name, build in E.MODELS.items():
        buf = build()
        xs = [E.model_input(buf, seed=60 + i) for i in range(5)]
        out[name] = (buf, xs, [run_reference(buf, x) for x in xs])
    return out


@pytest.mark.parametrize("all_tensors", [False, True], ids=["outputs", "every_tensor"])
@pytest.mark.parametrize("name", sorted(E.MODELS))
def test_models_gpu_executor(gpu_lib, monkeypatch, model_refs, name, all_tensors):
    """an eager pass, then the captured graph twice.  Outputs only: every
    LayerNorm is one layernorm_i8_kernel launch and none of its ten ops'.
    Every tensor viewed: nothing fused (two mean_rows_kernel and one
    eltwise_sqdiff_kernel launch per LayerNorm) and every intermediate compared."""
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf, xs, refs = model_refs[name]
    m, ex, key = _exec(buf, 81)
    om = OModel(buf)
    n_ln = E.LAYER_NORMS[name]
    kernels = [r["kernel"] for r in ex.ProfileSubgraph(key, iters=1)]
    assert kernels.count(E.LN_KERNEL) == n_ln, kernels
    assert E.MEAN_KERNEL not in kernels and E.SQDIFF_KERNEL not in kernels and "mean_kernel" not in kernels, kernels
    watch = list(ex.GetOutputs(key))
    if all_tensors:
        watch = [t.index for t in om.tensors if not t.is_const]
    views = {t: ex.GetTensorView(key, t) for t in watch}
    if all_tensors:
        kernels = [r["kernel"] for r in ex.ProfileSubgraph(key, iters=1)]
        assert E.LN_KERNEL not in kernels, kernels
        assert kernels.count(E.MEAN_KERNEL) == 2 * n_ln and kernels.count(E.SQDIFF_KERNEL) == n_ln, kernels
    t_in = ex.GetInputs(key)[0]
    for i in range(3):
        ex.GetTensorView(key, t_in).GetData()[...] = xs[i]
        assert ex.ExecuteSubgraph(key).ok()
        for t, v in views.items():
            np.testing.assert_array_equal(v.GetData().reshape(refs[i][t].shape), refs[i][t], err_msg="%s tensor %d" % (name, t))


@pytest.mark.parametrize("fusion", ["nolayernorm", "0"])
def test_models_without_the_fused_launch(gpu_lib, monkeypatch, model_refs, fusion):
    """BAND_HIP_FUSION=nolayernorm and =0: ten launches per LayerNorm, the outputs of the fused run"""
    monkeypatch.setenv("BAND_HIP_FUSION", fusion)
    buf, xs, refs = model_refs["encoder_17_48_3_96"]
    m, ex, key = _exec(buf, 82)
    kernels = [r["kernel"] for r in ex.ProfileSubgraph(key, iters=1)]
    assert E.LN_KERNEL not in kernels and kernels.count(E.MEAN_KERNEL) == 4 and kernels.count(E.SQDIFF_KERNEL) == 2, kernels
    t_in = ex.GetInputs(key)[0]
    for i in range(2):
        ex.GetTensorView(key, t_in).GetData()[...] = xs[i]
        assert ex.ExecuteSubgraph(key).ok()
        for t in ex.GetOutputs(key):
            np.testing.assert_array_equal(ex.GetTensorView(key, t).GetData().reshape(refs[i][t].shape), refs[i][t])


@pytest.mark.parametrize("which", sorted(E.LN_OP_OF))
def test_an_intermediate_that_is_a_model_output_keeps_the_ten_launches(gpu_lib, monkeypatch, which):
    """a LayerNorm whose row mean m, or whose a = x * g, is a model output beside y: the fused launch
    would not store it, so the ten ops stay ten launches, and every output is the bytes of the run
    with BAND_HIP_FUSION=nolayernorm"""
    buf = E.layer_norm_with_intermediate_output(which)
    xs = [E.model_input(buf, seed=70 + i) for i in range(2)]
    runs = {}
    for fusion in (None, "nolayernorm"):
        if fusion:
            monkeypatch.setenv("BAND_HIP_FUSION", fusion)
        else:
            monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
        m, ex, key = _exec(buf, 84)
        assert len(ex.GetOutputs(key)) == 2
        kernels = ex.LaunchKernels(key)
        t_in = ex.GetInputs(key)[0]
        outs = []
        for x in xs:
            ex.GetTensorView(key, t_in).GetData()[...] = x
            assert ex.ExecuteSubgraph(key).ok()
            outs.append([ex.GetTensorView(key, t).GetData().copy() for t in ex.GetOutputs(key)])
        runs[fusion] = (kernels, outs)
    kernels, outs = runs[None]
    assert len(kernels) == 10 and E.LN_KERNEL not in kernels, kernels
    assert kernels.count(E.MEAN_KERNEL) == 2 and kernels.count(E.SQDIFF_KERNEL) == 1, kernels
    assert kernels == runs["nolayernorm"][0]
    for got, ref in zip(outs, runs["nolayernorm"][1]):
        for g, r in zip(got, ref):
            assert g.tobytes() == r.tobytes()


@pytest.mark.parametrize("name", sorted(E.MODELS))
def test_models_job_batches(gpu_lib, monkeypatch, model_refs, name):
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf, xs, refs = model_refs[name]
    m, ex, key = _exec(buf, 83)
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
                    np.testing.assert_array_equal(got.reshape(refs[i][t].shape), refs[i][t],
                                                  err_msg="%s n=%d slot %d" % (name, n, s))


def test_engine_gpu_worker_only_serves_encoder_block(gpu_lib, tmp_path, monkeypatch):
    """one Band engine whose only worker is a GPU worker registers the encoder block and answers a request"""
    from band_amd.engine import Engine, JobStatus, Model, SchedulerType, make_config, kBandOk
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf = E.MODELS["encoder_17_48_3_96"]()
    x = E.model_input(buf, seed=9)
    ref = run_reference(buf, x)
    outputs = OModel(buf).outputs
    e = Engine(make_config([SchedulerType.kRoundRobin], [DeviceFlag.kGPU]))
    path = str(tmp_path / "encoder_block.tflite")
    with open(path, "wb") as f:
        f.write(buf)
    m = Model()
    assert m.FromPath(path)
    assert e.RegisterModel(m)
    t = e.CreateInputTensor(m, 0)
    t.data()[...] = x
    outs = [e.CreateOutputTensor(m, 0)]
    h = e.RequestAsync(m, [t])
    assert h >= 0 and e.Wait(h, outs) == kBandOk
    assert e.GetJobRecord(h).status == JobStatus.kSuccess
    np.testing.assert_array_equal(outs[0].data().reshape(ref[outputs[0]].shape), ref[outputs[0]])
    e.close()
