"""The LayerNorm / GELU ops without a GPU: the numpy restatements of
tests/encoder_models.py against the real-valued functions at derived bounds,
the C++ tables and host twins against the restatements bit for bit, the models
on the kCPU executor, the support checks and the synthesiser's old bytes."""
import ctypes
import hashlib
import math
import os
import subprocess

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi
from band_amd.tflite_reader_py import read
from band_amd.tflite_synth import OPT, ModelBuilder, Table, attention_block, vit_tiny
from tests import encoder_models as E
from tests.graph_reference import run_reference

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "band_amd", "csrc")
F = np.float32
MEAN_CASES = E.mean_cases()
SQDIFF_CASES = E.sqdiff_cases()


def _model(buf, mid=0):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    return m


# ---- the restatements against float64 -------------------------------------------------------
@pytest.mark.parametrize("q", E.RSQRT_Q)
def test_rsqrt_table_within_one_lsb_of_the_real_function(q):
    """Every entry with v = q - z_in > 0 is within 1 LSB of
    clip(1 / (sqrt(v s_in) s_out) + z_out): at most 0.5 from the final rounding
    plus the internal error.  Internal, relative to the unclamped value: the
    Newton iteration's fifth step leaves <= 1.3e-6 (start 1, worst target 2:
    relative errors .31, .13, .025, 9e-4, 1.3e-6), data = round(2^20 / sqrt(v))
    >= 65664 at v <= 255 adds <= 0.5 / 65664 = 7.6e-6, the Q31 multipliers
    2^-30 - together < 1e-5, i.e. < 0.003 LSB on a value of at most 255 + 128
    LSB inside the clamp; the second rounding of MultiplyByQuantizedMultiplier
    adds at most 2^-1 of a 2^-right-shift LSB.  Far below 0.5."""
    s_in, z_in, s_out, z_out = q
    table = E.np_rsqrt_table(*q).view(np.int8).astype(np.float64)
    worst = 0.0
    for code in range(-128, 128):
        v = code - z_in
        if v <= 0:
            assert table[code & 0xff] == 127
            continue
        real = 1.0 / (math.sqrt(v * float(F(s_in))) * float(F(s_out))) + z_out
        worst = max(worst, abs(table[code & 0xff] - min(max(real, -128.0), 127.0)))
    print("rsqrt", q, "worst", worst)
    assert worst <= 1.0
    assert len(np.unique(table)) >= 8, "the scales leave the table flat"


@pytest.mark.parametrize("q", E.GELU_Q)
@pytest.mark.parametrize("approximate", [False, True])
def test_gelu_table_within_one_lsb_of_the_real_function(q, approximate):
    """Within 1 LSB of clip(gelu(s_in (q - z_in)) / s_out + z_out): 0.5 from the
    rounding; internally four float32 roundings (the dequantised x, the
    transformed value, 1 / s_out, the product) of 2^-24 each on a value of at
    most 383 LSB, and |gelu'| <= 1.13 on x's rounding: < 1e-4 LSB."""
    signed, s_in, z_in, s_out, z_out = q
    table = E.np_gelu_table(signed, approximate, s_in, z_in, s_out, z_out)
    lo, hi = (-128, 127) if signed else (0, 255)
    worst = 0.0
    for code in range(lo, hi + 1):
        real = E.gelu_real(float(F(s_in)) * (code - z_in), approximate) / float(F(s_out)) + z_out
        got = int(table[code & 0xff].view(np.int8)) if signed else int(table[code])
        worst = max(worst, abs(got - min(max(real, lo), hi)))
    print("gelu", q, approximate, "worst", worst)
    assert worst <= 1.0
    assert len(np.unique(table)) >= 16


def test_gelu_forms_differ_and_match_known_values():
    """gelu(1) = 0.8413447 (exact form), 0.8411920 (tanh form); a swapped constant would miss them"""
    assert abs(E.gelu_real(1.0) - 0.8413447460685429) < 1e-12
    assert abs(E.gelu_real(1.0, True) - 0.8411919906082768) < 1e-9
    # x Phi(x) + x (1 - Phi(x)) = x
    assert abs(E.gelu_real(0.75) - E.gelu_real(-0.75) - 0.75) < 1e-12


@pytest.mark.parametrize("case", MEAN_CASES, ids=lambda c: c.name)
def test_mean_restatement_within_one_lsb(case):
    """Equal quantisation: the truncated quotient is within 1 (strictly) of the
    real mean.  Rescaled: r = round(y + 0.5) with y = mean s_in / s_out - z_in
    s_in / s_out, so r - z_out lies in (y, y + 1] before the float32 slack: four
    float32 roundings (the quotient, the scale, the product, the sum with the
    bias) on magnitudes of at most (255 + |z_in|) scale + 1 < 660 give
    4 x 2^-24 x 660 < 2e-4."""
    got = case.ref().astype(np.float64)
    mean = case.x.astype(np.float64).mean(-1)
    info = np.iinfo(case.dtype)
    (s_i, z_i), (s_o, z_o) = case.q_in, case.q_out
    real = np.clip((mean - z_i) * float(F(s_i)) / float(F(s_o)) + z_o, info.min, info.max)
    err = np.abs(got - real)
    print(case.name, "worst", err.max())
    assert err.max() <= 1.0 + (0.0 if case.exact else 2e-4)
    if case.exact and case.dtype == np.int8 and case.x.shape[0] > 2:
        s = int(case.x[2].astype(np.int64).sum())
        assert s < 0 and s % case.x.shape[1] != 0 and got[2] == -(-s // case.x.shape[1]), "truncation toward zero"


@pytest.mark.parametrize("case", SQDIFF_CASES, ids=lambda c: c.name)
def test_sqdiff_restatement_within_the_derived_bound(case):
    """With u = 2 max(s1, s2), each scaled input is a multiple of u / 128 off by
    at most 0.5 (+ 32640 x 2^-31 from the Q31 multiplier, 1.5e-5), so their
    difference d is off by at most 1 + 3e-5 units and d^2 by at most
    2 |d| (1 + 3e-5) + (1 + 3e-5)^2; one unit of d^2 is u^2 / (2^14 s_out)
    output LSB.  The output multiplier adds a relative 2^-30 and the output
    rounding 0.5; the clamp only shrinks the error."""
    (s1, z1), (s2, z2), (so, zo) = [(float(F(s)), z) for s, z in (case.q1, case.q2, case.qo)]
    u = 2.0 * max(s1, s2)
    ra, rb = (case.a.astype(np.float64) - z1) * s1, (case.b.astype(np.float64) - z2) * s2
    real = (ra - rb) ** 2 / so + zo
    d_units = np.abs(ra - rb) * 128.0 / u
    bound = (2.0 * d_units * (1 + 3e-5) + (1 + 3e-5) ** 2) * u * u / (16384.0 * so) + 0.5 + 1e-6 * np.abs(real)
    err = np.abs(case.ref().astype(np.float64) - np.clip(real, -128, 127))
    print(case.name, "worst error", err.max(), "bound there", bound.reshape(-1)[err.argmax()])
    assert (err <= bound).all()
    if case.name.startswith("extreme"):
        assert (case.ref() > -100).all() and (case.ref() < 127).all(), "the extremes must land inside the clamp"


# ---- C++ against numpy ----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def native(tmp_path_factory):
    """tests/native/layernorm_tables_test.cc with quant.cc, under AddressSanitizer and UBSan"""
    exe = str(tmp_path_factory.mktemp("ln") / "layernorm_tables_test")
    src = [os.path.join(ROOT, "tests", "native", "layernorm_tables_test.cc"), os.path.join(CSRC, "backend", "hip", "quant.cc")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                    "-I" + CSRC] + src + ["-o", exe], check=True, timeout=600)

    def run(*args):
        r = subprocess.run([exe] + [str(a) for a in args], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
        return r.stdout.splitlines()
    return run


def _hex(s):
    return float(F(s)).hex()


def test_native_tables_equal_numpy(native):
    args, want = [], []
    for s_in, z_in, s_out, z_out in E.RSQRT_Q:
        args += ["rsqrt", _hex(s_in), z_in, _hex(s_out), z_out]
        want.append(E.np_rsqrt_table(s_in, z_in, s_out, z_out))
    for signed, s_in, z_in, s_out, z_out in E.GELU_Q:
        for approx in (0, 1):
            args += ["gelu", int(signed), approx, _hex(s_in), z_in, _hex(s_out), z_out]
            want.append(E.np_gelu_table(signed, bool(approx), s_in, z_in, s_out, z_out))
    lines = native(*args)
    assert len(lines) == len(want)
    for ln, w in zip(lines, want):
        np.testing.assert_array_equal(np.array(ln.split(), np.int64), w.astype(np.int64))


def test_native_inverse_sqrt_and_sqdiff_params_equal_numpy(native):
    vs = list(range(1, 256)) + [1 << 20, (1 << 29) - 1, 1 << 29, (1 << 31) - 1]
    args = []
    for v in vs:
        args += ["invsqrt", v]
    for ln, v in zip(native(*args), vs):
        assert tuple(int(t) for t in ln.split()) == E.inv_sqrt_multiplier(v), v
    triples = [(c.q1[0], c.q2[0], c.qo[0]) for c in SQDIFF_CASES] + [(0.05, 0.05, 1e-7)]
    args = []
    for t in triples:
        args += ["sqdiff"] + [_hex(s) for s in t]
    for ln, t in zip(native(*args), triples):
        want = E.sqdiff_params(*t)
        if want is None:
            assert ln.startswith("refused: ") and "output multiplier >= 1" in ln, ln
        else:
            assert tuple(int(v) for v in ln.split()) == tuple(want) + (7,), (t, ln)


def test_library_tables_equal_numpy():
    """the same tables through the library the executors use"""
    lib = _abi.load()
    t = np.zeros(256, np.uint8)
    for q in E.RSQRT_Q:
        assert lib.bhx_rsqrt_table(q[0], q[1], q[2], q[3], t.ctypes.data) == 0
        np.testing.assert_array_equal(t, E.np_rsqrt_table(*q))
    for signed, s_in, z_in, s_out, z_out in E.GELU_Q:
        for approx in (0, 1):
            assert lib.bhx_gelu_table(int(signed), approx, s_in, z_in, s_out, z_out, t.ctypes.data) == 0
            np.testing.assert_array_equal(t, E.np_gelu_table(signed, bool(approx), s_in, z_in, s_out, z_out))


@pytest.mark.parametrize("case", MEAN_CASES, ids=lambda c: c.name)
def test_mean_rows_host_twin(case):
    np.testing.assert_array_equal(E.launch_mean(case, _abi.load(), False), case.ref())


@pytest.mark.parametrize("case", SQDIFF_CASES, ids=lambda c: c.name)
def test_sqdiff_host_twin(case):
    np.testing.assert_array_equal(E.launch_sqdiff(case, _abi.load(), False), case.ref())


def test_float_gelu_host_twin():
    """CpuUnaryF32 against float64 at E.gelu_f32_bound (glibc's erff / tanhf are within 1 ulp)"""
    lib = _abi.load()
    x = np.concatenate([np.linspace(-10, 10, 4001), [0.0, 1e-30, -1e-30, 1e-20, -1e-20]]).astype(F)
    y = np.zeros_like(x)
    for kind, approx in ((3, False), (4, True)):
        assert lib.bhx_cpu_unary_f32(kind, x.ctypes.data, y.ctypes.data, x.size) == 0
        ref = np.array([E.gelu_real(float(v), approx) for v in x])
        err = np.abs(y.astype(np.float64) - ref)
        tol = E.gelu_f32_bound(x, ref, 1)
        assert (err <= tol).all(), (x[err > tol][:5], err[err > tol][:5], tol[err > tol][:5])


# ---- models on the kCPU executor ----------------------------------------------------------------------
def non_constant_tensors(buf):
    return [i for i, t in enumerate(read(buf)["tensors"]) if t["data"] is None]


@pytest.fixture(scope="module")
def model_refs():
    out = {}
    for name, build in E.MODELS.items():
        buf = build()
        xs = [E.model_input(buf, seed=40 + s) for s in range(3)]
        out[name] = (buf, xs, [run_reference(buf, x) for x in xs])
    return out


@pytest.mark.parametrize("name", sorted(E.MODELS))
def test_models_on_cpu_executor_every_tensor(model_refs, name):
    buf, xs, refs = model_refs[name]
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    spec = ex.InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kCPU] == set() and spec.unsupported_ops[DeviceFlag.kGPU] == set()
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, 0)
    kinds = {o["builtin"] for o in read(buf)["ops"]}
    assert {E.MEAN, E.SQUARED_DIFFERENCE, E.RSQRT} <= kinds
    views = {t: ex.GetTensorView(key, t) for t in non_constant_tensors(buf)}
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = xs[0]
    assert ex.ExecuteSubgraph(key).ok()
    for t, v in views.items():
        np.testing.assert_array_equal(v.GetData().reshape(refs[0][t].shape), refs[0][t], err_msg="%s tensor %d" % (name, t))


def test_layer_norm_intermediates_are_spread_out(model_refs):
    """no LayerNorm tensor is flat or pinned to the clamp on the calibrated input spread, and the
    output tracks the float64 LayerNorm of the dequantised input"""
    buf, xs, refs = model_refs["layer_norm_5_48"]
    r = read(buf)
    for o in r["ops"]:
        t = o["outputs"][0]
        v = refs[0][t].astype(np.int32)
        if v.size >= 48:
            assert len(np.unique(v)) >= 8, (o["builtin"], t)
        assert ((v > -128) & (v < 127)).mean() >= 0.5 or o["builtin"] in (E.SQUARED_DIFFERENCE,), (o["builtin"], t)


def test_float_encoder_block_registers_and_runs():
    """the fp16-constant float32 block (float MEAN / SQUARED_DIFFERENCE / RSQRT / GELU) has no
    unsupported op on either worker and runs on the kCPU executor; its values are not held to a
    reference here (the float ops are, one by one, in the float tests and above)"""
    from band_amd.tflite_synth import encoder_block
    buf = encoder_block(np.float32, tokens=17, dim=48, heads=3, hidden=96)
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    spec = ex.InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kCPU] == set() and spec.unsupported_ops[DeviceFlag.kGPU] == set()
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(0, 0)
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = np.random.default_rng(0).normal(0, 1, (1, 17, 48))
    assert ex.ExecuteSubgraph(key).ok()
    assert np.isfinite(ex.GetTensorView(key, ex.GetOutputs(key)[0]).GetData()).all()


@pytest.mark.parametrize("n", [2, 3])
def test_job_batches_on_cpu(model_refs, n):
    buf, xs, refs = model_refs["encoder_17_48_3_96"]
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(0, 0)
    st = ex.PrepareJobBatches(m, key, 3)
    assert st.ok(), st.message()
    for s in range(n):
        ex.GetJobSlotView(key, ex.GetInputs(key)[0], n, s).GetData()[...] = xs[s]
    assert ex.ExecuteJobBatch(key, n).ok()
    for s in range(n):
        for t in ex.GetOutputs(key):
            np.testing.assert_array_equal(ex.GetJobSlotView(key, t, n, s).GetData().reshape(refs[s][t].shape), refs[s][t])


# ---- support checks --------------------------------------------------------------------------------------
def _one_op(kind, in_shapes, out_shape, dtype, options_type=0, options=None, extra_const=None, out_scale=0.05):
    mb = ModelBuilder("one_op")
    q = dict(scale=[0.05], zero_point=[128 if np.dtype(dtype) == np.uint8 else 0])
    ins = [mb.tensor("in%d" % i, list(s), dtype, **q) for i, s in enumerate(in_shapes)]
    mb.inputs += ins
    if extra_const is not None:
        ins.append(mb.tensor("axes", [len(extra_const)], np.int32, data=np.array(extra_const, np.int32)))
    y = mb.tensor("y", list(out_shape), dtype, scale=[out_scale], zero_point=q["zero_point"])
    mb.op(kind, ins, [y], options_type, options)
    mb.outputs.append(y)
    return mb.build()


REFUSALS = {
    "mean_axis_2": (lambda: _one_op("MEAN", [(1, 4, 6, 8)], (1, 4, 1, 8), np.int8, OPT["ReducerOptions"],
                                    Table().set(0, "b", 1), extra_const=[2]),
                    "8-bit MEAN: 4-D keep_dims over axes {1, 2}, or rank 1-4 over the last axis"),
    "sqdiff_uint8": (lambda: _one_op("SQUARED_DIFFERENCE", [(1, 4, 8), (1, 4, 8)], (1, 4, 8), np.uint8,
                                     OPT["SquaredDifferenceOptions"], Table()), "int8 and float32 only"),
    "sqdiff_multiplier": (lambda: _one_op("SQUARED_DIFFERENCE", [(1, 4, 8), (1, 4, 8)], (1, 4, 8), np.int8,
                                          OPT["SquaredDifferenceOptions"], Table(), out_scale=1e-7),
                          "output multiplier >= 1"),
    "gelu_int16": (lambda: _one_op("GELU", [(1, 4, 8)], (1, 4, 8), np.int16, OPT["GeluOptions"], Table().set(0, "b", 0)),
                   "GELU: int8, uint8 and float32 only"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_say_why(name):
    build, reason = REFUSALS[name]
    m = _model(build())
    spec = HipModelExecutor(0, 0, DeviceFlag.kCPU).InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kCPU] == {0} and spec.unsupported_ops[DeviceFlag.kGPU] == {0}
    st = HipModelExecutor(0, 0, DeviceFlag.kCPU).PrepareSubgraph(m)
    assert not st.ok() and reason in st.message(), st.message()


def test_mean_rows_refuses_bad_parameters():
    lib = _abi.load()
    x = np.zeros(64, np.uint8)
    for name, kw, reason in (("null_in", dict(input=None), "null pointer"), ("zero_rows", dict(rows=0), "non-positive"),
                             ("zero_depth", dict(depth=0), "non-positive"), ("float_type", dict(type=0), "type must be"),
                             ("row_sum", dict(depth=1 << 24), "depth * 255 >= 2^31")):
        p = _abi.MeanRowsParams()
        p.rows, p.depth, p.type, p.exact, p.input, p.output = 2, 8, 1, 1, x.ctypes.data, x.ctypes.data + 32
        for k, v in kw.items():
            setattr(p, k, v)
        assert lib.bh_mean_rows_check(ctypes.byref(p)) != 0, name
        msg = lib.bh_last_error().decode()
        assert msg.startswith("bh_mean_rows: ") and reason in msg, msg
        assert lib.bh_mean_rows_kernel(ctypes.byref(p)) == b""
        assert lib.bhx_cpu_mean_rows(ctypes.byref(p)) != 0


def test_layernorm_check_takes_the_lowered_blocks_and_refuses_long_rows():
    """bh_layernorm_i8_check (pure host) on the parameter blocks of a layer_norm model"""
    lib = _abi.load()
    x = np.zeros(64, np.uint8)
    ptr = x.ctypes.data
    p = E.LnCase(7, 64).params(ptr, ptr, ptr, ptr, ptr)
    assert lib.bh_layernorm_i8_check(ctypes.byref(p)) == 0, lib.bh_last_error()
    assert lib.bh_layernorm_i8_kernel(ctypes.byref(p)) == E.LN_KERNEL.encode()
    p = E.LnCase(3, 4100).params(ptr, ptr, ptr, ptr, ptr)
    assert lib.bh_layernorm_i8_check(ctypes.byref(p)) != 0
    assert "depth above 1024" in lib.bh_last_error().decode()


# ---- the synthesiser's old models keep their bytes -----------------------------------------------------
def test_default_models_keep_their_bytes():
    """sha256 of vit_tiny() and attention_block() with default arguments, recorded on the parent commit"""
    assert hashlib.sha256(vit_tiny()).hexdigest() == "895af68c210b3409ad6d9875f754ab327c7b75c19d92067c2fa07bca1c30b0d4"
    assert hashlib.sha256(attention_block()).hexdigest() == "3f35bd458a8d02ee0ab721205715f5c8f28a5e85c1df397fc6a274da0c63a232"
    assert hashlib.sha256(attention_block(np.float32)).hexdigest() == \
        "853f322b343ab39dc938171c0c115568acc856479bdafd162c55c350ab6839e7"
