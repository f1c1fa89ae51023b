"""ARG_MAX / ARG_MIN without a GPU: the reader, the support check, the kCPU
worker's host kernel (CpuArgMinMax; the kCPU worker lowers RESIZE_BILINEAR ->
ARG_MAX as two host kernels), job batching, and the test helper itself.
Expected outputs: the oracle's run of the model's twin without the tails,
then tests.argmax_models.arg_ref; everything compared with
assert_array_equal."""
import hashlib

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
from band_amd.tflite_synth import QGraph, deeplab_v3_mobilenet_v2
from tests.argmax_models import (arg_ref, argmax_zoo, argmax_zoo_ref, deeplab_logits, tied_pixels)


def _model(buf, mid=0):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    return m


def _run(buf, x, flag=DeviceFlag.kCPU, worker=0):
    m = _model(buf)
    ex = HipModelExecutor(0, worker, flag)
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, worker)
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = x
    assert ex.ExecuteSubgraph(key).ok()
    return [ex.GetTensorView(key, t).GetData().copy() for t in ex.GetOutputs(key)]


@pytest.fixture(scope="module")
def zoo_case():
    x = np.random.default_rng(7).integers(-128, 128, (1, 6, 5, 8)).astype(np.int8)
    return x, argmax_zoo_ref(x)


@pytest.fixture(scope="module")
def deeplab_case():
    x = np.random.default_rng(5).integers(-128, 128, (1, 64, 64, 3)).astype(np.int8)
    return x, deeplab_logits(64, x)


def test_reader_parses_both_ops_and_output_types():
    """builtin codes 56 / 79 in the file; the C++ reader names both ops (in the
    message of a refused lowering) and reads output_type: a tensor of either
    width is accepted exactly when output_type declares it"""
    from band_amd.tflite_reader_py import read
    assert sorted(o["builtin"] for o in read(argmax_zoo())["ops"] if o["builtin"] in (56, 79)) == [56, 56, 56, 79]
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    for minimum, name in ((False, "ARG_MAX"), (True, "ARG_MIN")):
        for out, code, other in ((np.int32, 2, 4), (np.int64, 4, 2)):
            ok = _model(_small(3, output=out, minimum=minimum))
            assert ex.InvestigateModelSpec(ok).unsupported_ops[DeviceFlag.kCPU] == set()
            bad = _model(_small(3, output=out, minimum=minimum, declared=other))
            assert ex.InvestigateModelSpec(bad).unsupported_ops[DeviceFlag.kCPU] == {1}
            st = HipModelExecutor(0, 0, DeviceFlag.kCPU).PrepareSubgraph(bad)
            assert not st.ok() and "(%s)" % name in st.message() and "output_type" in st.message()


@pytest.mark.parametrize("which", ["zoo", "deeplab32", "deeplab64"])
def test_no_unsupported_op_on_cpu(which):
    buf = {"zoo": argmax_zoo, "deeplab32": lambda: deeplab_v3_mobilenet_v2(np.int8, size=64, argmax=np.int32),
           "deeplab64": lambda: deeplab_v3_mobilenet_v2(np.int8, size=64, argmax=np.int64)}[which]()
    spec = HipModelExecutor(0, 0, DeviceFlag.kCPU).InvestigateModelSpec(_model(buf))
    assert spec.unsupported_ops[DeviceFlag.kCPU] == set()


def _small(axis, const_axis=True, output=np.int32, declared=None, minimum=False):
    """x [1, 4, 4, 3] -> conv -> ARG_MAX / ARG_MIN over `axis`; declared: another output_type"""
    g = QGraph(np.int8, seed=1, name="small")
    x = g.input([1, 4, 4, 3])
    y = g.conv(x, 5, k=1, act="NONE")
    out = g.arg_max(y, axis=axis, output=output, minimum=minimum)
    g.output(out)
    if not const_axis:
        g.mb.tensors[g.mb.ops[-1]["inputs"][1]]["buffer"] = 0  # the axis becomes a runtime tensor
        g.mb.inputs.append(g.mb.ops[-1]["inputs"][1])
    if declared is not None:
        g.mb.ops[-1]["options"].set(0, "b", declared)
    return g.build()


def test_unsupported_forms_say_why():
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    # a non-constant axis: unsupported on every worker, with the reason in the lowering error
    m = _model(_small(3, const_axis=False))
    spec = ex.InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kCPU] == {1}
    st = HipModelExecutor(0, 0, DeviceFlag.kCPU).PrepareSubgraph(m)
    assert not st.ok() and "ARG_MAX" in st.message() and "axis must be a constant" in st.message()
    # output tensor int32 under output_type int64
    m = _model(_small(3, declared=4))
    assert ex.InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kCPU] == {1}
    st = HipModelExecutor(0, 0, DeviceFlag.kCPU).PrepareSubgraph(m)
    assert not st.ok() and "output_type" in st.message()


def test_axis0_runs_but_refuses_job_batching():
    buf = _small(0)
    x = np.random.default_rng(3).integers(-128, 128, (1, 4, 4, 3)).astype(np.int8)
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kCPU] == set()
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(0, 0)
    st = ex.PrepareJobBatches(m, key, 3)
    assert not st.ok() and "ARG_MAX on the batch axis" in st.message()
    assert ex.MaxJobBatch(key) == 1
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = x
    assert ex.ExecuteSubgraph(key).ok()
    got = ex.GetTensorView(key, ex.GetOutputs(key)[0]).GetData()
    np.testing.assert_array_equal(got, np.zeros((4, 4, 5), np.int32))  # one element along axis 0


def test_zoo_on_cpu_executor(zoo_case):
    x, ref = zoo_case
    got = _run(argmax_zoo(), x)
    assert len(got) == len(ref)
    for g, r in zip(got, ref):
        assert g.dtype == r.dtype
        np.testing.assert_array_equal(g.reshape(r.shape), r)
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32


@pytest.mark.parametrize("out", [np.int32, np.int64])
def test_deeplab_argmax_on_cpu_executor(deeplab_case, out):
    x, logits = deeplab_case
    got = _run(deeplab_v3_mobilenet_v2(np.int8, size=64, argmax=out), x)
    assert len(got) == 1 and got[0].dtype == out and got[0].shape == (1, 64, 64)
    np.testing.assert_array_equal(got[0], arg_ref(logits, 3, out=out))


def test_job_batch_of_3_on_cpu(zoo_case, deeplab_case):
    rng = np.random.default_rng(11)
    for buf, shape, expect in (
            (argmax_zoo(), (1, 6, 5, 8), argmax_zoo_ref),
            (deeplab_v3_mobilenet_v2(np.int8, size=64, argmax=np.int32), (1, 64, 64, 3),
             lambda x: [arg_ref(deeplab_logits(64, x), 3)])):
        m = _model(buf)
        ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
        assert ex.PrepareSubgraph(m).ok()
        key = SubgraphKey(0, 0)
        st = ex.PrepareJobBatches(m, key, 3)
        assert st.ok(), st.message()
        xs = [rng.integers(-128, 128, shape).astype(np.int8) for _ in range(3)]
        for s, x in enumerate(xs):
            ex.GetJobSlotView(key, ex.GetInputs(key)[0], 3, s).GetData()[...] = x
        assert ex.ExecuteJobBatch(key, 3).ok()
        for s, x in enumerate(xs):
            ref = expect(x)
            for t, r in zip(ex.GetOutputs(key), ref):
                got = ex.GetJobSlotView(key, t, 3, s).GetData()
                np.testing.assert_array_equal(got.reshape(r.shape), r, err_msg="slot %d tensor %d" % (s, t))


def test_default_deeplab_bytes_unchanged():
    """argmax=None (bench.py's and every earlier test's model) is byte for byte
    what the synthesiser emitted before the argument existed (digests recorded
    from the parent commit)"""
    want = {(np.int8, 64): "3df691fb1f50a27194db86c5b6e3fe3cbeb67b97fdc2430d5a05a503f3c25231",
            (np.int8, 224): "04bcad42bac29f7e7200c464f5cc1750c9aede2c4fa843ca594f457f014e8b17",
            (np.uint8, 64): "84e3a1db452884f1ae19cdb0f16682bcd84759432eb0eb82ff942c8799c8668d"}
    for (dtype, size), digest in want.items():
        assert hashlib.sha256(deeplab_v3_mobilenet_v2(dtype, size=size)).hexdigest() == digest
        assert hashlib.sha256(deeplab_v3_mobilenet_v2(dtype, size=size, argmax=None)).hexdigest() == digest
    with pytest.raises(ValueError):
        deeplab_v3_mobilenet_v2(np.int8, size=64, argmax=np.int8)


def test_inputs_can_tell_a_wrong_tie_break(deeplab_case):
    """on the ORACLE's logits: >= 1,000 pixels of the size-64 model have a tied
    maximum whose first and last index differ (3,524 of 4,096 measured), so a
    last-index tie-break cannot pass the model tests"""
    _, logits = deeplab_case
    assert tied_pixels(logits) >= 1000
    assert (arg_ref(logits, 3) != logits.shape[3] - 1 - np.argmax(logits[..., ::-1], axis=3)).sum() >= 1000


def test_helper_rejects_wrong_semantics():
    # last-index tie-break
    row = np.array([[3, 9, 9, -4, 9]], np.int8)
    assert arg_ref(row, 1).tolist() == [1] and arg_ref(-row, 1, minimum=True).tolist() == [1]
    assert (row.shape[1] - 1 - np.argmax(row[:, ::-1], axis=1)).tolist() == [4]
    # a signed read of uint8: 0x80 is the maximum, 0x7f is not
    u = np.array([[0x7f, 0x80, 0x10]], np.uint8)
    assert arg_ref(u, 1).tolist() == [1] and arg_ref(u, 1, minimum=True).tolist() == [2]
    assert np.argmax(u.view(np.int8), axis=1).tolist() == [0] and np.argmin(u.view(np.int8), axis=1).tolist() == [1]
    # NaN is never greater or smaller: selected only as element 0
    f = np.array([[1.0, np.nan, 3.0, 2.0], [np.nan, 5.0, 7.0, 1.0], [-0.0, 0.0, -1.0, 0.0]], np.float32)
    assert arg_ref(f, 1).tolist() == [2, 0, 0] and arg_ref(f, 1, minimum=True).tolist() == [0, 0, 2]
    assert np.argmax(f, axis=1).tolist()[:2] == [1, 0]  # numpy's rule differs on row 0
    assert arg_ref(f, 1, out=np.int64).dtype == np.int64
    # a middle axis
    x = np.arange(24, dtype=np.int8).reshape(2, 3, 4)
    assert arg_ref(x, 1).shape == (2, 4) and (arg_ref(x, 1) == 2).all()
