"""Hybrid CONV_2D / DEPTHWISE_CONV_2D (float32 input, int8 filter) without a GPU.

First the numpy restatement of tests/hybrid_conv_models.py alone: against the
float64 convolution of the dequantised filter at the derived bound, against its
deliberately wrong variants, on directed items.  Then the host twins
(bhx_cpu_dynquant_items, bhx_cpu_conv_hybrid, bhx_cpu_dwconv_hybrid) on the
launcher cases, bit for bit; the launchers' refusals (pure host); the support
checks' reasons with BAND_HIP_HYBRID_CONV set and today's refusal without it;
the models on the kCPU executor with every tensor viewed; job batches; the
synthesiser's old bytes; the registration of a dynamic-range MobileNetV2."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi
from band_amd.tflite_synth import FGraph, encoder_block, mobilenet_v1, mobilenet_v2, vit_tiny
from oracle.tflite_fb import Model as OModel
from tests import float_harness as H
from tests import hybrid_conv_models as C

F = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DQ_CASES, CONV_CASES, DW_CASES = C.dq_cases(), C.conv_cases(), C.dw_cases()


@pytest.fixture
def hybrid_conv(monkeypatch):
    """executors constructed in the test run hybrid convolutions"""
    monkeypatch.setenv("BAND_HIP_HYBRID_CONV", "1")


def _model(buf, mid=0):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    return m


# ---- the restatement alone -----------------------------------------------------------------
JUDGED = [C.ConvCase("pt", 3, (7, 6), 5, 19, 3, seed=1), C.ConvCase("pt", 2, (8, 8), 16, 24, 3, stride=2, seed=2),
          C.ConvCase("pc", 3, (7, 6), 5, 19, 3, seed=3), C.ConvCase("pc", 2, (9, 8), 4, 12, 3, dilation=2, seed=4),
          C.ConvCase("pc", 2, (2, 2), 1280, 17, 1, seed=5), C.ConvCase("dw", 3, (7, 6), 16, 0, 3, seed=6),
          C.ConvCase("dw", 2, (6, 6), 5, 0, 5, stride=2, dm=2, seed=7)]


@pytest.mark.parametrize("case", JUDGED, ids=lambda c: c.name)
def test_reference_within_the_quantisation_bound(case):
    """|rule - float64 convolution of the dequantised filter| <= c s[b] ws[c] sum_in-bounds |w| +
    gamma(3) |y| (C.quantisation_bound); largest error / bound on these cases: 0.40 for one scale
    (symmetric items), 0.23 for out_c scales and 0.39 for depthwise (asymmetric items)"""
    real = C.real_conv(case.x, case.w, case.ws, case.bias, case.g, case.form, case.dm)
    got = case.ref().astype(np.float64)
    tol = C.quantisation_bound(case.x, case.w, case.ws, case.g, case.form, real, case.dm)
    ratio = np.abs(got - real) / tol
    print("hybrid conv reference %s: max error / bound %.3g" % (case.name, ratio.max()))
    assert (ratio <= 1.0).all()
    assert ratio.max() > 0.01  # the bound is not vacuous


def _border(case):
    """[OH, OW] bool: output pixels with at least one padded tap"""
    return C.in_bounds(case.in_hw, case.g).min(axis=(2, 3)) == 0


POS = {f: C.ConvCase(f, 2, (6, 6), 8, 0 if f == "dw" else 20, 3, x_mode="pos", seed=11) for f in ("pc", "dw")}
MIX = {f: C.ConvCase(f, 3, (6, 6), 8, 0 if f == "dw" else 20, 3, seed=12) for f in C.FORMS}


@pytest.mark.parametrize("form", ["pc", "dw"])
def test_wrong_padding_byte_differs_on_the_border(form):
    """all-positive items have off = -128; a padded tap filled with the byte 0 changes at least
    10 % of the border pixels' outputs (and no interior one)"""
    case = POS[form]
    assert (case.quantised()[2] == -128).all()
    ref, bad = case.ref(), case.ref("pad_zero")
    border = _border(case)
    assert border.any() and not border.all()
    share = float((ref != bad)[:, border].mean())
    print("wrong variant pad_zero %s: %.3f of the border outputs differ" % (form, share))
    assert share >= 0.10
    np.testing.assert_array_equal(ref[:, ~border], bad[:, ~border])


@pytest.mark.parametrize("form,wrong", [("pc", "no_rowsum"), ("dw", "no_rowsum"), ("pt", "per_row"), ("pc", "per_row"),
                                        ("dw", "per_row"), ("pc", "swap"), ("dw", "swap"), ("pt", "fma"), ("pc", "fma"),
                                        ("dw", "fma")])
def test_wrong_variants_differ(form, wrong):
    """each wrong variant changes at least 10 % of the outputs (measured with numpy: no row-sum
    term and per-row quantisation 1.0, the exchanged epilogue orders 0.29 - 0.33, one FMA
    0.26 - 0.27)"""
    case = MIX[form]
    share = float((case.ref() != case.ref(wrong)).mean())
    print("wrong variant %s %s: %.3f of the outputs differ" % (wrong, form, share))
    assert share >= 0.10


@pytest.mark.parametrize("form", C.FORMS)
def test_whole_batch_quantisation_differs(form):
    """items of different ranges: one quantisation for the batch changes at least 10 % of the
    outputs of every item whose range is not the widest"""
    case = MIX[form]
    _, s, _ = case.quantised()
    narrow = s < s.max()
    assert narrow.sum() == case.batch - 1
    share = float((case.ref() != case.ref("whole_batch"))[narrow].mean())
    print("wrong variant whole_batch %s: %.3f of the narrower items' outputs differ" % (form, share))
    assert share >= 0.10


@pytest.mark.parametrize("form", ["pc", "dw"])
def test_first_channel_scale_for_all_differs(form):
    """ws[0] for every channel changes at least 10 % of the outputs of the other channels"""
    case = MIX[form]
    diff = case.ref() != case.ref("ws0")
    assert not diff[..., 0].any()
    assert float(diff[..., 1:].mean()) >= 0.10


def test_reference_directed_items():
    """per item: offset -128 on an all-positive item, 127 on an all-negative one, an interior
    value on a mixed one; a zero item gives s = 1 and q = 0"""
    rng = np.random.default_rng(3)
    x = rng.normal(0, 1, (4, 3, 4, 5)).astype(F)
    x[0] = np.abs(x[0]) + F(0.25)
    x[1] = -np.abs(x[1]) - F(0.25)
    x[3] = 0
    q, s, off = C.np_dynquant_items(x, True)
    assert off[0] == -128 and off[1] == 127 and -128 < off[2] < 127
    assert s[3] == 1 and off[3] == 0 and (q[3] == 0).all()
    q, s, off = C.np_dynquant_items(x, False)
    assert (off == 0).all() and s[3] == 1 and (q[3] == 0).all()
    assert (np.abs(q.astype(int)).reshape(4, -1).max(axis=1)[:3] == 127).all()
    # an item is one row: rows of the same item share s and off although their own ranges differ
    assert len({float(v) for v in s[:3]}) == 3


# ---- the host twins -------------------------------------------------------------------------
@pytest.mark.parametrize("case", DQ_CASES, ids=lambda c: c.name)
def test_dynquant_items_host_twin(case):
    q, s, off = C.launch_dq(case, _abi.load(), False)
    rq, rs, roff = case.ref()
    np.testing.assert_array_equal(q, rq, err_msg=case.name + " q")
    np.testing.assert_array_equal(s, rs, err_msg=case.name + " scale")
    np.testing.assert_array_equal(off, roff, err_msg=case.name + " offset")


@pytest.mark.parametrize("case", CONV_CASES + DW_CASES, ids=lambda c: c.name)
def test_conv_host_twins(case):
    q, s, off, y = C.launch_conv(case, _abi.load(), False)
    rq, rs, roff = case.quantised()
    np.testing.assert_array_equal(q, rq, err_msg=case.name + " q")
    np.testing.assert_array_equal(s, rs, err_msg=case.name + " scale")
    np.testing.assert_array_equal(off, roff, err_msg=case.name + " offset")
    np.testing.assert_array_equal(y, case.ref(), err_msg=case.name)


def test_launcher_cases_cover_the_issue():
    conv = CONV_CASES
    assert {c.K for c in conv} >= {1, 15, 16, 17, 27, 63, 64, 65, 130, 1280}
    assert {c.in_c for c in conv} >= {1, 3, 4, 5, 16} and {c.out_c for c in conv} >= set(C.OUT_CS) | {1001}
    assert {c.M for c in conv} >= {1, 15, 16, 17, 65}
    assert {c.form for c in conv} == {"pt", "pc"} and {c.act for c in conv} == set(C.ACTS)
    assert {c.bias is None for c in conv} == {False, True}
    assert any(c.batch == 3 and c.g.out_hw == (3, 3) for c in conv)
    assert any(c.M <= 16 and c.K > 128 for c in conv) and any(c.g.dilation == (2, 2) for c in conv)
    offs = np.concatenate([c.quantised()[2] for c in conv + DW_CASES if c.form != "pt"])
    assert offs.min() == -128 and offs.max() == 127 and ((offs > -128) & (offs < 127)).any()
    dw = DW_CASES
    assert {c.in_c for c in dw} >= {1, 3, 4, 5, 16, 130} and {c.dm for c in dw} == {1, 2}
    assert {c.g.k_hw for c in dw} >= {(3, 3), (5, 5)} and {c.g.stride for c in dw} >= {(1, 1), (2, 2)}
    assert {c.act for c in dw} == set(C.ACTS) and any(c.batch == 3 for c in dw)
    sizes = {c.size for c in DQ_CASES}
    assert sizes >= set(C.DQ_SIZES) and {c.batch for c in DQ_CASES} == {1, 3}
    assert {c.form for c in DQ_CASES} == {0, 1, 2} and {c.kernel() for c in DQ_CASES} == {C.DQ_ONE, C.DQ_TWO}


def _refusals(lib, who, check, kernel, cpu, which, cases, ptr):
    for name, kw, reason in cases:
        p = C.valid_blocks(ptr)[which]
        assert check(ctypes.byref(p)) == 0, lib.bh_last_error()
        for k, v in kw.items():
            setattr(p, k, v)
        assert check(ctypes.byref(p)) != 0, name
        msg = lib.bh_last_error().decode()
        assert msg.startswith(who + ": ") and reason in msg, msg
        assert kernel(ctypes.byref(p)) == b"", name
        assert cpu(ctypes.byref(p)) != 0, name
    assert check(None) != 0


def test_launchers_refuse_bad_parameters():
    """the three *_check functions are pure host; the host twins refuse the same"""
    lib = _abi.load()
    keep = C.Y.AlignedHost(np.zeros(4096, np.uint8))
    _refusals(lib, "bh_dynquant_items", lib.bh_dynquant_items_check, lib.bh_dynquant_items_kernel,
              lib.bhx_cpu_dynquant_items, 0, C.DQ_REFUSALS, keep.value)
    _refusals(lib, "bh_conv2d_hybrid", lib.bh_conv2d_hybrid_check, lib.bh_conv2d_hybrid_kernel, lib.bhx_cpu_conv_hybrid, 1,
              C.CONV_REFUSALS, keep.value)
    _refusals(lib, "bh_dwconv2d_hybrid", lib.bh_dwconv2d_hybrid_check, lib.bh_dwconv2d_hybrid_kernel,
              lib.bhx_cpu_dwconv_hybrid, 2, C.DW_REFUSALS, keep.value)


def test_host_twins_under_sanitizers(tmp_path):
    """tests/native/conv_hybrid_twins_test.cc: a stand-alone program that runs the three twins on a
    few cases (padding, stride 2, dilation, a depth multiplier, a K that is no multiple of 16)
    against a plain restatement, under AddressSanitizer and UBSan"""
    csrc = os.path.join(ROOT, "band_amd", "csrc")
    exe = str(tmp_path / "conv_hybrid_twins_test")
    src = [os.path.join(ROOT, "tests", "native", "conv_hybrid_twins_test.cc"),
           ] + [os.path.join(csrc, "backend", "hip", f) for f in ("cpu_kernels.cc", "quant.cc")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(csrc, "compat"), "-I" + csrc] + src + ["-o", exe, "-lpthread"], check=True,
                   timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "cases ok" in r.stdout, r.stdout


# ---- support checks ---------------------------------------------------------------------------
# (the two 2^31-element models are left to tests/test_lower_args_hybrid_conv_cpu.py, which asks
# HybridConvArgs itself: an executor sizes its tensor table for them first, which takes 20 s)
@pytest.mark.parametrize("name", sorted(n for n in C.REFUSALS if not n.endswith("_elements")))
def test_refusals_say_why(hybrid_conv, name):
    build, reason = C.REFUSALS[name]
    m = _model(build())
    spec = HipModelExecutor(0, 0, DeviceFlag.kCPU).InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kCPU] == {0} and spec.unsupported_ops[DeviceFlag.kGPU] == {0}
    st = HipModelExecutor(0, 0, DeviceFlag.kCPU).PrepareSubgraph(m)
    assert not st.ok() and reason in st.message(), st.message()


@pytest.mark.parametrize("depthwise", [False, True], ids=["conv", "depthwise"])
def test_flag_unset_refuses_with_todays_reason(monkeypatch, depthwise):
    """without BAND_HIP_HYBRID_CONV (or with a value that is not 1) an op the flag would accept is
    refused by both workers' sets, with the reason of before"""
    for value in (None, "0", "yes"):
        if value is None:
            monkeypatch.delenv("BAND_HIP_HYBRID_CONV", raising=False)
        else:
            monkeypatch.setenv("BAND_HIP_HYBRID_CONV", value)
        m = _model(C.raw_model(depthwise))
        spec = HipModelExecutor(0, 0, DeviceFlag.kCPU).InvestigateModelSpec(m)
        assert spec.unsupported_ops[DeviceFlag.kCPU] == {0} and spec.unsupported_ops[DeviceFlag.kGPU] == {0}
        st = HipModelExecutor(0, 0, DeviceFlag.kCPU).PrepareSubgraph(m)
        assert not st.ok() and st.message().endswith(": " + C.TODAY), st.message()
    monkeypatch.setenv("BAND_HIP_HYBRID_CONV", "1")
    assert HipModelExecutor(0, 0, DeviceFlag.kCPU).PrepareSubgraph(_model(C.raw_model(depthwise))).ok()


def test_flag_is_latched_at_construction(monkeypatch):
    monkeypatch.setenv("BAND_HIP_HYBRID_CONV", "1")
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    monkeypatch.delenv("BAND_HIP_HYBRID_CONV")
    assert ex.PrepareSubgraph(_model(C.raw_model(False))).ok()


# ---- models on the kCPU executor ------------------------------------------------------------
def test_dynamic_range_mobilenet_registers(hybrid_conv):
    """the dynamic-range MobileNetV2 is in nobody's unsupported_ops and PrepareSubgraph succeeds
    (before hybrid CONV_2D / DEPTHWISE_CONV_2D: every large convolution refused by both workers)"""
    m = _model(C.REGISTRATION())
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    spec = ex.InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kCPU] == set() and spec.unsupported_ops[DeviceFlag.kGPU] == set()
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    kernels = ex.LaunchKernels(SubgraphKey(0, 0))
    assert kernels.count("conv_hybrid_host") >= 30 and kernels.count("dwconv_hybrid_host") >= 1
    assert kernels.count("dynquant_items_host") == kernels.count("conv_hybrid_host") + kernels.count("dwconv_hybrid_host")


@pytest.mark.parametrize("name", sorted(C.MODELS))
def test_models_on_cpu_executor_every_tensor(hybrid_conv, name):
    buf = C.MODELS[name]()
    om, runs = H.run_executor(buf, [C.model_feed(buf, seed=11)], DeviceFlag.kCPU, 0, view_all=True)
    hybrid = sum(C.is_hybrid_conv(om, o) for o in om.operators)
    assert hybrid >= 1
    assert H.check_graph_ops(om, runs[0], name, gelu_ulps=1)[1]["conv"] == hybrid
    assert all(np.isfinite(v).all() for v in runs[0].values())


def test_launch_kernels_of_one_op_models(hybrid_conv):
    for name, want in (("conv_pt_2x7x6x5", "conv_hybrid_host"), ("dw_2x7x6x8", "dwconv_hybrid_host")):
        ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
        assert ex.PrepareSubgraph(_model(C.MODELS[name]())).ok()
        assert ex.LaunchKernels(SubgraphKey(0, 0)) == ["dynquant_items_host", want]


@pytest.mark.parametrize("n", [2, 3])
def test_job_batches_on_cpu(hybrid_conv, n):
    """each job of a batch equals its own single-job run: every item is quantised alone"""
    buf = C.MODELS[C.BATCHED]()
    feeds = [{t: v * F(1 + 2 * s) for t, v in C.model_feed(buf, seed=20 + s).items()} for s in range(n)]
    om, singles = H.run_executor(buf, feeds, DeviceFlag.kCPU, 0, view_all=False)
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(0, 0)
    st = ex.PrepareJobBatches(m, key, 3)
    assert st.ok(), st.message()
    for s in range(n):
        ex.GetJobSlotView(key, ex.GetInputs(key)[0], n, s).GetData()[...] = feeds[s][om.inputs[0]]
    assert ex.ExecuteJobBatch(key, n).ok()
    for s in range(n):
        for t in om.outputs:
            np.testing.assert_array_equal(ex.GetJobSlotView(key, t, n, s).GetData().reshape(singles[s][t].shape),
                                          singles[s][t], err_msg="job %d of %d" % (s, n))


# ---- the synthesiser ---------------------------------------------------------------------------
DIGESTS = {  # sha256 of models built without the new keywords, recorded on the parent commit
    "encoder_block_f32": (lambda: encoder_block(np.float32),
                          "0dc98cd831d52ff7b7fa340748fc8508d52fde48678d42698b8dd13ed0bf2358"),
    "encoder_block_hybrid": (lambda: encoder_block(np.float32, tokens=17, dim=48, heads=3, hidden=96, hybrid="symmetric"),
                             "a6412b619718e73ba21c5eb8931bdc25ee78f5aabd6d8682585f30720943d855"),
    "mobilenet_v1_f16_32": (lambda: mobilenet_v1(np.float16, size=32),
                            "0d6dc5cd6e35475d12741940c0c8392f9f4fb6dfc5e5d25c834f33a65b62b026"),
    "mobilenet_v1_u8_32": (lambda: mobilenet_v1(np.uint8, size=32),
                           "c56074ce432b73d152a27a668129883fd563624e27f08e7035ba690986c9bd04"),
    "mobilenet_v2_f16_32": (lambda: mobilenet_v2(np.float16, size=32),
                            "d8d0fad961785a6bb8f248eac18a77b0ff9a7e44b1f0132e504c8764031caacc"),
    "mobilenet_v2_i8_32": (lambda: mobilenet_v2(np.int8, size=32),
                           "c5573365c7cfdfa393099bc259df70bc0de867c38619e7141dea3bb0a95fe0bc"),
    "vit_tiny_hybrid_asym_32": (lambda: vit_tiny(np.float32, size=32, dim=48, heads=3, blocks=1, hybrid="asymmetric"),
                                "c492aedc60e7b7385ccbc82daae42110dd34ccd6faeb440cc2e5ae5385215600"),
    "vit_tiny_hybrid_sym_32": (lambda: vit_tiny(np.float32, size=32, dim=48, heads=3, layer_norm=True, mlp=True,
                                                hybrid="symmetric"),
                               "aa9d11ff3b92a7f5e170d670790573f2a04e422aed8bdee027a13994b2d1556d"),
    "vit_tiny_i8_32": (lambda: vit_tiny(np.int8, size=32, dim=48),
                       "ac28ab83d6eec0efd55ee60610a164da5a77ef781ad3d205bb2fff640f294d08"),
}


@pytest.mark.parametrize("name", sorted(DIGESTS))
def test_existing_models_keep_their_bytes(name):
    build, digest = DIGESTS[name]
    assert hashlib.sha256(build()).hexdigest() == digest


def test_synthesised_hybrid_convs():
    """int8 filters with ws = max|w| / 127 per output channel (dimension 0, 3 for depthwise) or for
    the whole filter, zero points 0, plain float32 biases, no DEQUANTIZE; small filters stay float32"""
    for form in C.FORMS:
        om = OModel(C.one_op_model(form, (1, 6, 6, 4), 9))
        (o,) = om.operators
        w, b = om.tensors[o.inputs[1]], om.tensors[o.inputs[2]]
        out_c = w.shape[3] if form == "dw" else w.shape[0]
        assert w.np_dtype == np.int8 and w.is_const and len(w.scale) == (1 if form == "pt" else out_c)
        assert all(int(z) == 0 for z in w.zero_point) and b.np_dtype == np.float32 and b.is_const
        mags = np.abs(w.data.astype(int))
        if form == "pt":
            assert mags.max() == 127
        else:
            assert w.quantized_dimension == (3 if form == "dw" else 0)
            assert (mags.max(axis=(0, 1, 2) if form == "dw" else (1, 2, 3)) == 127).all()
    for min_elements, floats in ((0, 0), (1024, None)):
        om = OModel(mobilenet_v2(np.float32, size=32, classes=21, hybrid_conv="per_channel", hybrid_min_elements=min_elements))
        convs = [o for o in om.operators if o.builtin in (C.CONV_2D, C.DEPTHWISE_CONV_2D)]
        assert all(o.name != "DEQUANTIZE" for o in om.operators) and len(convs) == 53
        kept = [o for o in convs if not C.is_hybrid_conv(om, o)]
        assert all(om.tensors[o.inputs[1]].np_dtype == np.float32 for o in kept)
        assert all(int(np.prod(om.tensors[o.inputs[1]].shape)) < min_elements for o in kept)
        assert all(int(np.prod(om.tensors[o.inputs[1]].shape)) >= min_elements for o in convs if o not in kept)
        if floats is not None:
            assert len(kept) == floats
        else:
            assert 1 <= len(kept) < len(convs)
    om = OModel(C.MODELS["vit_tiny_32"]())
    assert C.is_hybrid_conv(om, om.operators[0]) and all(o.name != "DEQUANTIZE" for o in om.operators)
    g = FGraph(seed=1)
    with pytest.raises(AssertionError):
        g.conv(g.input([1, 4, 4, 4]), 2, hybrid="per-row")
