"""HybridConvArgs (backend/hip/lower_args.{h,cc}), the one function the support
checks, the lowering and job batching share for hybrid CONV_2D /
DEPTHWISE_CONV_2D: its classifications (form, input quantisation, geometry,
expanded scales) and each of its refusals with the reason, in a stand-alone
program (tests/native/hybrid_conv_args_test.cc) under AddressSanitizer and
UBSan, linked with the TFLite reader and nothing of the executor; and the same
classification as the kCPU executor lowers it."""
import os
import subprocess

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
from oracle.tflite_fb import Model as OModel
from tests import hybrid_conv_models as C

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "band_amd", "csrc")

ACCEPTED = {
    "conv_pt": (lambda: C.one_op_model("pt", (2, 7, 6, 5), 19, k=3, stride=2, act="RELU6"),
                "ok conv per_tensor symmetric in 2x7x6x5 out 4x3x19 k 3x3 stride 2 dil 1 pad 1,0 dm 1 act 3 bias 1"),
    "conv_pc": (lambda: C.one_op_model("pc", (1, 9, 8, 4), 12, k=3, dilation=2, bias=False),
                "ok conv per_channel asymmetric in 1x9x8x4 out 9x8x12 k 3x3 stride 1 dil 2 pad 2,2 dm 1 act 0 bias 0"),
    "conv_one_channel": (lambda: C.one_op_model("pc", (1, 4, 4, 4), 1, k=1),
                         "ok conv per_tensor symmetric in 1x4x4x4 out 4x4x1 k 1x1"),
    "dw": (lambda: C.one_op_model("dw", (3, 6, 6, 3), k=5, stride=2, dm=2, padding="VALID"),
           "ok depthwise per_channel asymmetric in 3x6x6x3 out 1x1x6 k 5x5 stride 2 dil 1 pad 0,0 dm 2 act 0 bias 1"),
    "dw_one_channel": (lambda: C.raw_model(True, in_shape=(1, 4, 4, 1), out_c=1, w_scale=[0.01]),
                       "ok depthwise per_channel asymmetric in 1x4x4x1 out 4x4x1"),
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    """lines printed by the sanitizer build of the driver over every model"""
    tmp = tmp_path_factory.mktemp("hybrid_conv_args")
    models = {name: build() for name, (build, _) in C.REFUSALS.items()}
    models.update({name: build() for name, (build, _) in ACCEPTED.items()})
    paths = []
    for name, buf in models.items():
        paths.append(str(tmp / (name + ".tflite")))
        with open(paths[-1], "wb") as f:
            f.write(buf)
    exe = str(tmp / "hybrid_conv_args_test")
    src = [os.path.join(ROOT, "tests", "native", "hybrid_conv_args_test.cc")]
    src += [os.path.join(CSRC, "backend", "hip", f) for f in ("tflite_reader.cc", "lower_args.cc", "quant.cc")]
    src.append(os.path.join(CSRC, "compat", "band", "common.cc"))
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(CSRC, "compat"), "-I" + CSRC] + src +
                   ["-o", exe], check=True, timeout=600)
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    return r.stdout.splitlines()


def _line(lines, name):
    hit = [ln for ln in lines if "/%s.tflite op 0 " % name in ln]
    assert len(hit) == 1, (name, hit)
    return hit[0].split(": ", 1)[1]


@pytest.mark.parametrize("name", sorted(C.REFUSALS))
def test_refusal_reasons(driver, name):
    got = _line(driver, name)
    assert got.startswith(C.REFUSALS[name][1]), got


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_classifications(driver, name):
    build, want = ACCEPTED[name]
    got = _line(driver, name)
    assert got.startswith(want), got
    om = OModel(build())
    w = om.tensors[om.operators[0].inputs[1]]
    first, last = got.rsplit("scales ", 1)[1].split()
    assert np.float32(first) == np.float32(w.scale[0]) and np.float32(last) == np.float32(w.scale[-1])


@pytest.mark.parametrize("name", sorted(ACCEPTED))
def test_the_lowering_takes_the_same_form(monkeypatch, name):
    """the kCPU executor lowers what HybridConvArgs classified: its launches, and an output that is the
    rule's for that form bit for bit"""
    monkeypatch.setenv("BAND_HIP_HYBRID_CONV", "1")
    buf = ACCEPTED[name][0]()
    m = HipModel(0)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    spec = ex.InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kCPU] == set() and spec.unsupported_ops[DeviceFlag.kGPU] == set()
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(0, 0)
    dw = name.startswith("dw")
    assert ex.LaunchKernels(key) == ["dynquant_items_host", "dwconv_hybrid_host" if dw else "conv_hybrid_host"]
    om = OModel(buf)
    feed = C.model_feed(buf, seed=5)
    ex.GetTensorView(key, om.inputs[0]).GetData()[...] = feed[om.inputs[0]]
    assert ex.ExecuteSubgraph(key).ok()
    got = ex.GetTensorView(key, om.outputs[0]).GetData()
    ref = C.hybrid_conv_reference(om, om.operators[0], feed[om.inputs[0]])
    np.testing.assert_array_equal(got.reshape(ref.shape), ref)
