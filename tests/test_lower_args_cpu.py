"""The Args functions of the conv / FC / pool / eltwise families
(backend/hip/lower_args.h) as the support checks and the lowering use them:
malformed models are refused by both workers' support sets and by
PrepareSubgraph with the same reason, and a graph through every family runs
bit-exact against the oracle, at batch 1 and as a job-batch variant (whose
output-shape checks see the scaled batch axis)."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
from tests import lower_args_models as L
from tests import reindex_models as R
from tests.graph_reference import run_reference
from tests.test_float_cpu import assert_float_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(L.MALFORMED))
def test_malformed_model_is_refused_with_the_reason(name):
    """prepared in a child process: the op is in unsupported_ops of kCPU and
    kGPU, PrepareSubgraph names the Args function's reason, the child exits
    normally (before the Args functions the stride-0 pool died of SIGFPE)"""
    _, op, reason = L.MALFORMED[name]
    r = subprocess.run([sys.executable, "-m", "tests.lower_args_models", name], cwd=ROOT, capture_output=True,
                       text=True, timeout=120)
    assert r.returncode == 0, (r.returncode, r.stderr[-2000:])
    got = json.loads(r.stdout.strip().splitlines()[-1])
    # (kGPU also lists a DEQUANTIZE whose only reader it refuses: the placement rule of InvestigateModelSpec)
    assert got["cpu"] == [op] and op in got["gpu"], got
    assert not got["ok"], got
    assert "HIP backend cannot run op %d" % op in got["message"] and reason in got["message"], got["message"]


def _model(buf):
    m = HipModel(0)
    assert m.FromBuffer(buf).ok()
    return m


@pytest.fixture(scope="module")
def families():
    buf = L.families()
    xs = [R.zoo_input(buf, seed=40 + s) for s in range(2)]
    return buf, xs, [run_reference(buf, x) for x in xs]


def test_families_model_bit_exact_on_cpu(families):
    buf, xs, refs = families
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    spec = ex.InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kCPU] == set() and spec.unsupported_ops[DeviceFlag.kGPU] == set()
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, 0)
    kernels = ex.LaunchKernels(key)
    # every family lowered to its own launch; one ADD folded, one did not
    for want in ("conv_grouped_host", "zero_insert_kernel", "pool_kernel", "eltwise_kernel", "fc_kernel"):
        assert any(k.startswith(want) for k in kernels), (want, kernels)
    assert sum(k.endswith("+add") for k in kernels) == 1 and kernels.count("eltwise_kernel") == 2, kernels
    assert sum(k.startswith("dwconv") for k in kernels) == 2, kernels
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = xs[0]
    assert ex.ExecuteSubgraph(key).ok()
    t = ex.GetOutputs(key)[0]
    assert len(np.unique(refs[0][t])) >= 5
    np.testing.assert_array_equal(ex.GetTensorView(key, t).GetData().reshape(refs[0][t].shape), refs[0][t])


def test_families_model_every_tensor_on_cpu(families):
    """with every tensor viewed nothing folds: each op's own output against the oracle"""
    buf, xs, refs = families
    from tests.test_grouped_conv_cpu import non_constant_tensors
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(0, 0)
    views = {t: ex.GetTensorView(key, t) for t in non_constant_tensors(buf)}
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = xs[0]
    assert ex.ExecuteSubgraph(key).ok()
    for t, v in views.items():
        np.testing.assert_array_equal(v.GetData().reshape(refs[0][t].shape), refs[0][t], err_msg="tensor %d" % t)


def test_families_model_as_job_batch_variant(families):
    buf, xs, refs = families
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(0, 0)
    st = ex.PrepareJobBatches(m, key, 2)
    assert st.ok(), st.message()
    assert ex.MaxJobBatch(key) == 2
    for s, x in enumerate(xs):
        ex.GetJobSlotView(key, ex.GetInputs(key)[0], 2, s).GetData()[...] = x
    assert ex.ExecuteJobBatch(key, 2).ok()
    t = ex.GetOutputs(key)[0]
    for s in range(2):
        np.testing.assert_array_equal(ex.GetJobSlotView(key, t, 2, s).GetData().reshape(refs[s][t].shape), refs[s][t])


def test_float_families_model_on_cpu():
    """the float32 forms take their geometry from the same functions: against
    the oracle's float interpreter at the tolerance of tests/test_float_cpu.py
    (an fp16-weight graph has no job-batch variants: its DEQUANTIZE outputs
    are tensors without a batch axis)"""
    from oracle.runner import OracleInterpreter
    from oracle.tflite_fb import Model as OModel
    buf = L.float_families()
    om = OModel(buf)
    rng = np.random.default_rng(50)
    x = rng.uniform(-1, 1, om.tensors[om.inputs[0]].shape).astype(np.float32)
    ref = OracleInterpreter(om).run({om.inputs[0]: x})[om.outputs[0]]
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kCPU] == set()
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, 0)
    t = ex.GetOutputs(key)[0]
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = x
    assert ex.ExecuteSubgraph(key).ok()
    assert len(np.unique(ref)) == ref.size
    assert_float_close(ex.GetTensorView(key, t).GetData().reshape(ref.shape), ref, "float families")
