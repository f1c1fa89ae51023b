"""TANH and EMBEDDING_LOOKUP without a GPU (CAST and the padded text models: tests/test_cast_mask_*.py): the 8-bit TANH
table and the float32 host twin against tests.tanh_lookup_models' references,
EMBEDDING_LOOKUP through tests.gather_models' axis-0 cases on the kCPU executor,
the refusals with their reasons, the text models with a pooler and an
EMBEDDING_LOOKUP on the kCPU executor with every tensor viewed, job batches, and
the host code under AddressSanitizer / UBSan as a stand-alone program."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi
from oracle.tflite_fb import Model as OModel
from tests import gather_models as G
from tests import tanh_lookup_models as T
from tests.graph_reference import claimants, run_reference
from tests.test_float_cpu import assert_float_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _model(buf, mid=0):
    from band_amd import backend  # noqa: F401
    m = HipModel(mid)
    st = m.FromBuffer(buf)
    assert st.ok(), st.message()
    return m


def _run(buf, feeds):
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, 0)
    for t, x in zip(ex.GetInputs(key), feeds):
        ex.GetTensorView(key, t).GetData()[...] = x
    assert ex.ExecuteSubgraph(key).ok()
    return [ex.GetTensorView(key, t).GetData().copy() for t in ex.GetOutputs(key)], ex.LaunchKernels(key)


# ---- TANH ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("q", T.TANH_Q, ids=["%s_%g" % ("i8" if q[0] else "u8", q[1]) for q in T.TANH_Q])
def test_tanh_table_all_256_bytes(q):
    from band_amd import backend  # noqa: F401
    lib = _abi.load()
    signed, s_in, z_in, s_out, z_out = q
    t = np.zeros(256, np.uint8)
    assert lib.bhx_tanh_table(int(signed), s_in, z_in, s_out, z_out, t.ctypes.data) == 0
    want = T.np_tanh_table(signed, s_in, z_in, s_out, z_out)
    np.testing.assert_array_equal(t, want)
    vals = want.view(np.int8).astype(int) if signed else want.astype(int)
    assert len(np.unique(vals)) >= 16  # no constant table: 0.25 per LSB over +-32 leaves 24 distinct values


def test_tanh_tables_reach_both_ends_at_the_wide_scale():
    want = T.np_tanh_table(True, 0.25, -20, 1.0 / 128, 0).view(np.int8)
    assert want.min() == -128 and want.max() == 127


@pytest.mark.parametrize("q", T.TANH_Q[:2], ids=["i8", "u8"])
def test_one_tanh_model_is_the_table(q):
    signed, s_in, z_in, s_out, z_out = q
    dt = np.int8 if signed else np.uint8
    x = np.arange(256, dtype=np.uint8).view(dt).reshape(1, 4, 64)
    (got,), kernels = _run(T.raw_tanh((1, 4, 64), dt, in_q=(s_in, z_in), out_q=(s_out, z_out)), [x])
    assert kernels == ["lut_u8_kernel"]
    np.testing.assert_array_equal(got.reshape(-1).view(np.uint8), T.np_tanh_table(*q)[x.reshape(-1).view(np.uint8)])


def test_float32_tanh_host_twin():
    """|got - tanh(x)| <= gamma(k) |y| + 2^-126 against float64 tanh, k = 4: glibc states 2 ulp for tanhf and an ulp
    is at most 2 u |y| (tests.tanh_lookup_models.tanh_f32_bound).  Observed: 0.60 of the bound at the worst input."""
    from band_amd import backend  # noqa: F401
    lib = _abi.load()
    x = T.tanh_f32_inputs()
    out = np.zeros_like(x)
    assert lib.bhx_cpu_unary_f32(6, x.ctypes.data, out.ctypes.data, x.size) == 0
    ref = np.tanh(x.astype(np.float64))
    err = np.abs(out.astype(np.float64) - ref)
    tol = T.tanh_f32_bound(ref, "host")
    print("float32 TANH (host): largest |error| / bound %.3f" % (err / tol).max())
    assert (err <= tol).all()
    for kind in (5, 7):  # BH_UNARY_TANH is 6: 5 stays no kind
        assert lib.bhx_cpu_unary_f32(kind, x.ctypes.data, out.ctypes.data, x.size) != 0


def test_one_float32_tanh_model():
    x = T.tanh_f32_inputs()[:4096].reshape(1, 64, 64)
    (got,), kernels = _run(T.raw_tanh((1, 64, 64), np.float32, in_q=None, out_q=None), [x])
    assert kernels == ["unary_f32_kernel"]
    ref = np.tanh(x.astype(np.float64))
    assert (np.abs(got.reshape(ref.shape).astype(np.float64) - ref) <= T.tanh_f32_bound(ref, "host")).all()


# ---- EMBEDDING_LOOKUP ----------------------------------------------------------------------------
AXIS0 = [c for c in G.launcher_cases() if c.axis == 0 and not c.int64_only and c.misalign == 0]


@pytest.mark.parametrize("index_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("case", AXIS0, ids=[c.name for c in AXIS0])
def test_embedding_lookup_on_the_gather_cases(case, index_dtype):
    """gather_models' axis-0 cases, the out-of-range ones among them, as one-op EMBEDDING_LOOKUP models with runtime
    ids: np.take, a zero row for an id outside the table"""
    buf = T.raw_lookup(case.shape, case.indices, case.dtype, index_dtype=index_dtype)
    (got,), kernels = _run(buf, [np.asarray(case.indices, index_dtype)])
    assert kernels == ["gather_host"]
    np.testing.assert_array_equal(got.reshape(case.ref().shape), case.ref())


def test_embedding_lookup_of_an_activation_table_by_constant_ids_is_refused_for_batching_only():
    buf = T.raw_lookup((1, 16), [0, 0], runtime_ids=False, const_table=False)
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.PrepareSubgraph(m).ok()
    st = ex.PrepareJobBatches(m, SubgraphKey(0, 0), 2)
    assert not st.ok() and "job batching: EMBEDDING_LOOKUP with an activation params gathered along the batch axis" in st.message()


# ---- refusals ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(T.REFUSALS))
def test_refusals_say_why(name):
    build, reason = T.REFUSALS[name]
    m = _model(build())
    for flag in (DeviceFlag.kCPU, DeviceFlag.kGPU):
        ex = HipModelExecutor(0, 0 if flag == DeviceFlag.kCPU else 1, flag)
        spec = ex.InvestigateModelSpec(m)
        assert spec.unsupported_ops[flag] != set(), name
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    st = ex.PrepareSubgraph(m)
    assert not st.ok() and reason in st.message(), st.message()


# ---- models ----------------------------------------------------------------------------------------------
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
        buf = build()
        x = T.token_ids(buf, seed=3)
        out[name] = (buf, x, run_reference(buf, x, table=T.REF_TABLE))
    return out


@pytest.mark.parametrize("name", sorted(T.TEXT_MODELS))
def test_text_models_on_cpu_executor_every_tensor(model_refs, name):
    buf, x, ref = model_refs[name]
    om = OModel(buf)
    assert {T.TANH, T.EMBEDDING_LOOKUP} <= {o.builtin for o in om.operators} and G.GATHER not in {o.builtin for o in om.operators}
    for o in om.operators:
        if o.builtin in (T.TANH, T.EMBEDDING_LOOKUP):
            assert claimants(om, o, T.REF_TABLE) == [len(T.REF_TABLE) - 1]
            assert len(np.unique(ref[o.outputs[0]])) >= 8
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    spec = ex.InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kCPU] == set() and spec.unsupported_ops[DeviceFlag.kGPU] == set()
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, 0)
    views = {t.index: ex.GetTensorView(key, t.index) for t in om.tensors if not t.is_const}
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = x
    assert ex.ExecuteSubgraph(key).ok()
    for t, v in views.items():
        _compare(name, t, v.GetData(), ref[t])


def test_pooler_output_quantisation():
    om = OModel(T.TEXT_MODELS["text_pooler_i8"]())
    tanh = next(o for o in om.operators if o.builtin == T.TANH)
    t = om.tensors[tanh.outputs[0]]
    assert (float(t.scale[0]), int(t.zero_point[0])) == (1.0 / 128, 0) and tuple(t.shape) == (2, 48)


def test_existing_text_encoder_bytes_are_unchanged():
    import hashlib
    from band_amd.tflite_synth import text_encoder
    from tests.test_attention_mask_cpu import DIGESTS
    buf = text_encoder(np.int8, tokens=17, dim=48, heads=3, hidden=96, vocab=128, batch=2)
    assert hashlib.sha256(bytes(buf)).hexdigest() == DIGESTS["text_encoder_i8"]


@pytest.mark.parametrize("name", ["text_pooler_i8", "text_pooler_hybrid"])
def test_text_models_job_batches_on_cpu(name):
    buf = T.TEXT_MODELS[name](batch=1)
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(0, 0)
    st = ex.PrepareJobBatches(m, key, 3)
    assert st.ok(), st.message()
    t_in = ex.GetInputs(key)[0]
    xs = [T.token_ids(buf, seed=s) for s in range(3)]
    refs = [run_reference(buf, x, table=T.REF_TABLE) for x in xs]
    for n in (2, 3):
        for s in range(n):
            ex.GetJobSlotView(key, t_in, n, s).GetData()[...] = xs[s]
        assert ex.ExecuteJobBatch(key, n).ok()
        for s in range(n):
            for t in ex.GetOutputs(key):
                _compare(name, t, ex.GetJobSlotView(key, t, n, s).GetData().reshape(refs[s][t].shape), refs[s][t])


# ---- sanitizers ----------------------------------------------------------------------------------------------
def test_host_code_under_sanitizers(tmp_path):
    """tests/native/tanh_lookup_test.cc: a stand-alone program that runs TanhTable over its scales, CpuUnaryF32's
    TANH on exactly sized buffers and EmbeddingLookupArgs / TanhArgs on hand-built models, under AddressSanitizer
    and UBSan"""
    csrc = os.path.join(ROOT, "band_amd", "csrc")
    models = {name: build() for name, (build, _) in T.REFUSALS.items()}
    models["good_tanh"] = T.raw_tanh()
    models["good_lookup"] = T.raw_lookup((9, 16), [8, 0, 3])
    paths = []
    for name, buf in models.items():
        paths.append(str(tmp_path / (name + ".tflite")))
        with open(paths[-1], "wb") as f:
            f.write(buf)
    exe = str(tmp_path / "tanh_lookup_test")
    src = [os.path.join(ROOT, "tests", "native", "tanh_lookup_test.cc")] + [
        os.path.join(csrc, "backend", "hip", f) for f in ("tflite_reader.cc", "lower_args.cc", "quant.cc", "cpu_kernels.cc")]
    src.append(os.path.join(csrc, "compat", "band", "common.cc"))
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(csrc, "compat"), "-I" + csrc] + src + ["-o", exe, "-lpthread"], check=True,
                   timeout=600)
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "tanh lookup ok" in r.stdout, r.stdout
    lines = r.stdout.splitlines()
    for name, (_, reason) in T.REFUSALS.items():
        hit = [ln for ln in lines if "/%s.tflite op 0 " % name in ln]
        assert len(hit) == 1 and reason in hit[0], (name, hit)
    for name in ("good_tanh", "good_lookup"):
        assert [ln for ln in lines if "/%s.tflite op 0 " % name in ln and ln.endswith(": ok")], lines
