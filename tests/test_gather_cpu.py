"""GATHER, PACK, UNPACK and TILE without a GPU: CpuGather through the C ABI on
the launcher case table and on extreme indices, the support checks' refusals
with their reasons, text_encoder and the PACK / UNPACK / TILE zoo on the kCPU
executor with every tensor compared, the job-batch rules, and the synthesiser.

The reference is numpy (tests/gather_models.py) and
tests.graph_reference.run_reference with the family's table entries.  Integer
tensors are compared with assert_array_equal, float tensors with
assert_float_close of tests/test_float_cpu.py."""
import ctypes
import hashlib
import os
import subprocess

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi
from band_amd.tflite_reader_py import OPTION_FIELDS, read
from band_amd.tflite_synth import OPT, attention_block, encoder_block, text_encoder, vit_tiny
from oracle.tflite_fb import Model as OModel
from tests import gather_models as G
from tests.graph_reference import TABLE, claimants, run_reference
from tests.test_float_cpu import assert_float_close

REF_TABLE = TABLE + G.ENTRIES
CASES = [(c, dt) for c in G.launcher_cases() for dt in (np.int32, np.int64) if dt == np.int64 or not c.int64_only]
IDS = ["%s-%s" % (c.name, np.dtype(dt).name) for c, dt in CASES]


def _model(buf, mid=0):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    return m


# ---- the reference ---------------------------------------------------------------------
def test_gather_ref_is_np_take_in_range_and_zero_outside():
    x = G.fill((3, 7, 5), np.uint8)
    idx = np.array([[6, 0], [3, 3]])
    np.testing.assert_array_equal(G.gather_ref(x, idx, 1), np.take(x, idx, 1))
    np.testing.assert_array_equal(G.gather_ref(x, idx, -1 + 2), np.take(x, idx, 1))
    got = G.gather_ref(x, [7, 2, -1], 1)
    assert got.shape == (3, 3, 5) and not got[:, 0].any() and not got[:, 2].any()
    np.testing.assert_array_equal(got[:, 1], x[:, 2])
    assert x.min() > 0 and (x != G.GUARD_BYTE).all()  # a zero slice and a guard row are no table row


# ---- CpuGather through the C ABI ---------------------------------------------------------
@pytest.mark.parametrize("case,index_dtype", CASES, ids=IDS)
def test_cpu_gather_launcher_cases(case, index_dtype):
    lib = _abi.load()
    want = case.ref()
    got = G.run_cpu_gather(lib, case, index_dtype)
    np.testing.assert_array_equal(got.reshape(want.shape), want)
    raw, at = case.guarded_table()
    p = G.gather_params(case, index_dtype, raw.ctypes.data + at, raw.ctypes.data, raw.ctypes.data)
    if at % case.dtype.itemsize == 0:
        assert lib.bh_gather_kernel(ctypes.byref(p)).decode() == G.KERNEL


EXTREMES = {np.int32: [-2**31, 2**31 - 1, -1, 9], np.int64: [2**32 + 1, -2**32 + 2, 2**40, -2**63, 2**63 - 1]}


@pytest.mark.parametrize("index_dtype", [np.int32, np.int64])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_extreme_indices_give_zero_slices(dtype, index_dtype):
    """INT32_MIN, INT32_MAX, -1 and axis_size; 2^32 + 1, -2^32 + 2 (which narrow to rows 1 and 2) and 2^40:
    zero slices, the rows between them right, through the range function the kernel shares"""
    lib = _abi.load()
    case = G.Case("extremes", dtype, (9, 16), 0, [0])
    idx = []
    for v in EXTREMES[index_dtype]:
        idx += [v, 3]
    got = G.run_cpu_gather(lib, case, index_dtype, idx)
    x = case.params()
    assert got.shape == (1, len(idx), 16)
    for j, v in enumerate(idx):
        if v == 3:
            np.testing.assert_array_equal(got[0, j], x[3], err_msg="neighbour of %d" % idx[j - 1])
        else:
            assert not got[0, j].view(np.uint8).any(), "index %d" % v


def test_cpu_gather_refuses_what_the_launcher_refuses():
    lib = _abi.load()
    buf = np.zeros(256, np.uint8)
    a = buf.ctypes.data + (-buf.ctypes.data) % 16
    ok = dict(elem_bytes=4, index_bytes=4, outer=1, axis_size=4, n_idx=2, inner=4, params=a, indices=a + 128,
              output=a + 64)
    assert lib.bh_gather_check(ctypes.byref(_abi.GatherParams(**ok))) == 0
    for bad, reason in ((dict(params=None), "non-null"), (dict(indices=None), "non-null"), (dict(output=None), "non-null"),
                        (dict(elem_bytes=2), "elem_bytes must be 1 or 4"), (dict(index_bytes=2), "index_bytes must be 4 or 8"),
                        (dict(params=a + 2), "aligned to elem_bytes"), (dict(indices=a + 130), "aligned to index_bytes"),
                        (dict(n_idx=0), "invalid parameters"),
                        (dict(n_idx=1 << 20, inner=1 << 9), "more than 2^31 - 1 output bytes"),
                        (dict(outer=1 << 31), "more than 2^31 - 1 output bytes")):
        p = _abi.GatherParams(**dict(ok, **bad))
        assert lib.bh_gather_check(ctypes.byref(p)) != 0
        msg = lib.bh_last_error().decode()
        assert msg.startswith("bh_gather: ") and reason in msg, msg
        assert lib.bh_gather_kernel(ctypes.byref(p)) == b""
        assert lib.bhx_cpu_gather(ctypes.byref(p)) != 0
    # 2^31 - 1 bytes exactly is the largest accepted size
    assert lib.bh_gather_check(ctypes.byref(_abi.GatherParams(**dict(ok, elem_bytes=1, n_idx=2**31 - 1, inner=1)))) == 0


def test_a_map_with_indices_goes_to_the_gather():
    """bh_reindex_params.indices: CpuReindex and bh_reindex_kernel hand the map to the gather; a map of another form,
    the canonicaliser and a null-index map are unchanged"""
    lib = _abi.load()
    for case in [c for c in G.launcher_cases() if c.name in ("outer3_axis1_float32", "out_of_range_u8", "u8_row1040")]:
        want = case.ref()
        x = case.params()
        idx = np.asarray(case.indices, np.int32)
        out = np.full(want.nbytes + 16, 0xff, np.uint8)
        p = G.indexed_map(case, np.int32, x.ctypes.data, idx.ctypes.data, out.ctypes.data)
        assert lib.bh_reindex_kernel(ctypes.byref(p)).decode() == G.KERNEL
        assert lib.bhx_cpu_reindex(ctypes.byref(p)) == 0, lib.bhx_last_error()
        np.testing.assert_array_equal(out[:want.nbytes].view(case.dtype).reshape(want.shape), want)
        assert (out[want.nbytes:] == 0xff).all()
        assert lib.bh_reindex_canonical(ctypes.byref(p), ctypes.byref(_abi.ReindexParams())) != 0
        assert b"no canonical form" in lib.bh_last_error()
        p.in_stride[1] += 1  # not [outer][index_range][inner]
        assert lib.bh_reindex_kernel(ctypes.byref(p)) == b"" and lib.bhx_cpu_reindex(ctypes.byref(p)) != 0


def test_host_twin_under_sanitizers(tmp_path):
    """tests/native/gather_twin_test.cc: a stand-alone program that runs CpuGather on exactly sized buffers, the
    extreme indices among them, under AddressSanitizer and UBSan"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    csrc = os.path.join(root, "band_amd", "csrc")
    exe = str(tmp_path / "gather_twin_test")
    src = [os.path.join(root, "tests", "native", "gather_twin_test.cc"),
           ] + [os.path.join(csrc, "backend", "hip", f) for f in ("cpu_kernels.cc", "quant.cc")]
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(root, "include"),
                    "-I" + os.path.join(csrc, "compat"), "-I" + csrc] + src + ["-o", exe, "-lpthread"], check=True,
                   timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "gather twin ok" in r.stdout, r.stdout


# ---- support and refusals ----------------------------------------------------------------
REFUSALS = {
    "batch_dims_1": (lambda: G.raw_gather((2, 4, 8), [[0, 1], [2, 3]], axis=1, batch_dims=1, out_shape=[2, 2, 8]),
                     "GATHER batch_dims != 0"),
    "requantising": (lambda: G.raw_gather((4, 8), [1, 2], out_scale=0.25), "GATHER never requantises"),
    "constant_index_too_large": (lambda: G.raw_gather((4, 8), [1, 4]), "GATHER constant index outside [0, axis_size)"),
    "constant_index_negative": (lambda: G.raw_gather((4, 8), [-1, 2], index_dtype=np.int64),
                                "GATHER constant index outside [0, axis_size)"),
    "output_shape": (lambda: G.raw_gather((4, 8), [1, 2], out_shape=[1, 2, 8]), "GATHER output shape differs"),
    "float16_params": (lambda: G.raw_gather((4, 8), [1, 2], dtype=np.float16), "GATHER params must be int8"),
    "tile_rank7": (lambda: G.raw_tile((2, 2, 2, 2), (2, 2, 2, 1)), "TILE map exceeds rank 6"),
    "tile_runtime_multiples": (lambda: _tile_with_runtime_multiples(), "TILE multiples must be a constant"),
    "pack_17_inputs": (lambda: G.raw_pack(17), "PACK of more than 16 inputs"),
    "pack_mismatched_quantisation": (lambda: G.raw_pack(3, odd_scale_at=1), "PACK inputs must share the output's quantization"),
}


def _tile_with_runtime_multiples():
    from band_amd.tflite_synth import ModelBuilder, Table
    mb = ModelBuilder("raw_tile")
    x = mb.tensor("x", [1, 4], np.int8, scale=[0.5], zero_point=[3])
    mt = mb.tensor("multiples", [2], np.int32)
    mb.inputs += [x, mt]
    y = mb.tensor("y", [1, 8], np.int8, scale=[0.5], zero_point=[3])
    mb.op("TILE", [x, mt], [y], OPT["TileOptions"], Table())
    mb.outputs.append(y)
    return mb.build()


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_say_why(name):
    """the op is in unsupported_ops of both workers, and the lowering error names the reason"""
    build, reason = REFUSALS[name]
    m = _model(build())
    spec = HipModelExecutor(0, 0, DeviceFlag.kCPU).InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kCPU] == {0} and spec.unsupported_ops[DeviceFlag.kGPU] == {0}
    st = HipModelExecutor(0, 0, DeviceFlag.kCPU).PrepareSubgraph(m)
    assert not st.ok() and reason in st.message(), st.message()


def _run(buf, feeds, flag=DeviceFlag.kCPU, worker=0):
    m = _model(buf)
    ex = HipModelExecutor(0, worker, flag)
    assert ex.InvestigateModelSpec(m).unsupported_ops[flag] == set()
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, worker)
    for t, x in zip(ex.GetInputs(key), feeds):
        ex.GetTensorView(key, t).GetData()[...] = x
    assert ex.ExecuteSubgraph(key).ok()
    return [ex.GetTensorView(key, t).GetData().copy() for t in ex.GetOutputs(key)], ex.LaunchKernels(key)


ONE_OP = [  # params shape, indices, axis, dtype
    ((5, 6), [4, 0, 4], 0, np.int8), ((5, 6), [[4, 0], [2, 2]], 0, np.uint8), ((3, 7, 5), [6, 0, 3], 1, np.float32),
    ((3, 7, 5), [4, 4, 0], -1, np.int32), ((2, 3, 4, 5, 6), [[1], [3]], 3, np.int8), ((7,), 2, 0, np.float32),
]


@pytest.mark.parametrize("runtime", [False, True], ids=["constant_indices", "runtime_indices"])
@pytest.mark.parametrize("index_dtype", [np.int32, np.int64])
def test_one_gather_models_are_np_take(index_dtype, runtime):
    for shape, idx, axis, dtype in ONE_OP:
        x = G.fill(shape, dtype)
        want = np.take(x, idx, axis)
        buf = G.raw_gather(shape, idx, axis, dtype=dtype, runtime_indices=runtime, index_dtype=index_dtype)
        feeds = [x] + ([np.asarray(idx, index_dtype)] if runtime else [])
        (got,), kernels = _run(buf, feeds)
        assert kernels == ["gather_host"] and got.dtype == dtype
        np.testing.assert_array_equal(got.reshape(want.shape), want, err_msg=str((shape, idx, axis)))


def test_runtime_index_out_of_range_is_a_zero_slice_and_the_pass_succeeds():
    x = G.fill((5, 6), np.int8)
    buf = G.raw_gather((5, 6), [0, 0, 0, 0], runtime_indices=True, index_dtype=np.int64)
    (got,), _ = _run(buf, [x, np.array([5, 1, -1, 2**32 + 3], np.int64)])
    np.testing.assert_array_equal(got.reshape(4, 6), G.gather_ref(x, [5, 1, -1, 2**32 + 3]))
    assert not got.reshape(4, 6)[[0, 2, 3]].any() and got.reshape(4, 6)[1].all()


def test_identity_gather_is_a_copy():
    """outer 1 and the constant indices 0 .. axis_size - 1: the bytes of params, as LowerReindex makes of the identity"""
    x = G.fill((5, 6), np.int8)
    (got,), kernels = _run(G.raw_gather((5, 6), [0, 1, 2, 3, 4]), [x])
    assert kernels == ["copy"]
    np.testing.assert_array_equal(got.reshape(5, 6), x)
    (got,), kernels = _run(G.raw_gather((5, 6), [0, 1, 2, 4, 3]), [x])
    assert kernels == ["gather_host"]
    np.testing.assert_array_equal(got.reshape(5, 6), x[[0, 1, 2, 4, 3]])
    (got,), kernels = _run(G.raw_gather((2, 3, 4), [0, 1, 2], axis=1), [G.fill((2, 3, 4), np.int8)])
    assert kernels == ["gather_host"]  # outer 2: the same bytes, but the rule is outer == 1


@pytest.mark.parametrize("name,shape,multiples,kernel", G.TILE_MAPS, ids=[t[0] for t in G.TILE_MAPS])
@pytest.mark.parametrize("dtype", [np.uint8, np.float32])
def test_tile_is_np_tile(name, shape, multiples, kernel, dtype):
    x = G.fill(shape, dtype)
    (got,), kernels = _run(G.raw_tile(shape, multiples, dtype, np.int64 if dtype == np.float32 else np.int32), [x])
    np.testing.assert_array_equal(got.reshape(np.tile(x, multiples).shape), np.tile(x, multiples))
    assert kernels == ["reindex_host"]
    # the map the device would run, by kernel: a pure function of the map
    assert _tile_kernel(shape, multiples, dtype) == kernel


def _tile_kernel(shape, multiples, dtype):
    lib = _abi.load()
    p = G.tile_map(shape, multiples, dtype, 0, 0)
    return lib.bh_reindex_kernel(ctypes.byref(p)).decode()


@pytest.mark.parametrize("name,shape,multiples,kernel", G.TILE_MAPS, ids=[t[0] for t in G.TILE_MAPS])
def test_cpu_reindex_takes_zero_strides(name, shape, multiples, kernel):
    lib = _abi.load()
    x = G.fill(shape, np.uint8)
    want = np.tile(x, multiples)
    out = np.full(want.nbytes + 16, 0xff, np.uint8)
    p = G.tile_map(shape, multiples, np.uint8, x.ctypes.data, out.ctypes.data)
    assert lib.bhx_cpu_reindex(ctypes.byref(p)) == 0, lib.bhx_last_error()
    np.testing.assert_array_equal(out[:want.nbytes].reshape(want.shape), want)
    assert (out[want.nbytes:] == 0xff).all()


@pytest.mark.parametrize("dtype", [np.int8, np.float32])
def test_pack_and_unpack_one_op_models(dtype):
    xs = [G.fill((2, 4, 8), dtype) + dtype(k) for k in range(3)]
    for axis in (0, 1, 2, 3, -1):
        mb_axis = axis if axis >= 0 else axis + 4
        (got,), kernels = _run(G.raw_pack(3, (2, 4, 8), mb_axis, dtype), xs)
        want = np.stack(xs, axis)
        np.testing.assert_array_equal(got.reshape(want.shape), want, err_msg="PACK axis %d" % axis)
        assert kernels == ["concat_kernel"]
    x = G.fill((2, 3, 4, 8), dtype)
    for axis in (0, 1, 2, 3):
        got, kernels = _run(G.raw_unpack((2, 3, 4, 8), axis, dtype), [x])
        want = G.unpack_ref(x, axis)
        assert len(got) == len(want) == x.shape[axis]
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g.reshape(w.shape), w, err_msg="UNPACK axis %d" % axis)


# ---- whole models --------------------------------------------------------------------------
def _compare(name, t, got, ref):
    assert got.dtype == ref.dtype, (name, t)
    if ref.dtype == np.float32:
        assert_float_close(got, ref, "%s tensor %d" % (name, t))
    else:
        np.testing.assert_array_equal(got.reshape(ref.shape), ref, err_msg="%s tensor %d" % (name, t))


@pytest.fixture(scope="module")
def model_refs():
    out = {}
    for name, build in G.TEXT_ENCODERS.items():
        buf = build()
        x = G.token_ids(buf, seed=3)
        out[name] = (buf, x, run_reference(buf, x, table=REF_TABLE))
    for name, build in G.ZOO.items():
        buf = build()
        x = G.zoo_input(buf, seed=3)
        out[name] = (buf, x, run_reference(buf, x, table=REF_TABLE))
    return out


@pytest.mark.parametrize("name", sorted(G.TEXT_ENCODERS) + sorted(G.ZOO))
def test_models_on_cpu_executor_every_tensor(model_refs, name):
    buf, x, ref = model_refs[name]
    om = OModel(buf)
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
    assert {o.builtin for o in om.operators} & G.OPS
    for t, v in views.items():
        _compare(name, t, v.GetData(), ref[t])


def test_the_family_claims_its_ops_alone(model_refs):
    for name, (buf, x, ref) in model_refs.items():
        om = OModel(buf)
        for o in om.operators:
            assert len(claimants(om, o, REF_TABLE)) <= 1
            if o.builtin in G.OPS:
                assert claimants(om, o, REF_TABLE) == [len(TABLE)]
                for t in o.outputs:  # what the ops move is no constant: a wrong row would show
                    assert len(np.unique(ref[t])) >= 8, (name, t)


# ---- job batching ----------------------------------------------------------------------------
def test_the_embedding_model_batches_on_cpu():
    buf = G.TEXT_ENCODERS["text_encoder_i8"]()
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(0, 0)
    st = ex.PrepareJobBatches(m, key, 3)
    assert st.ok(), st.message()
    assert ex.MaxJobBatch(key) == 3
    t_in = ex.GetInputs(key)[0]
    xs = [G.token_ids(buf, seed=10 + s) for s in range(3)]
    for s, x in enumerate(xs):
        ex.GetJobSlotView(key, t_in, 3, s).GetData()[...] = x
    assert ex.ExecuteJobBatch(key, 3).ok()
    for s, x in enumerate(xs):
        ref = run_reference(buf, x, table=REF_TABLE)
        for t in ex.GetOutputs(key):
            np.testing.assert_array_equal(ex.GetJobSlotView(key, t, 3, s).GetData().reshape(ref[t].shape), ref[t])


S4 = (1, 4, 4, 8)
BATCH_RULES = {
    "gather_activation_runtime_indices": (lambda: G.raw_gather(S4, [1, 2], axis=1, runtime_indices=True),
                                          "job batching: GATHER with runtime indices into an activation params"),
    "gather_activation_axis0": (lambda: G.raw_gather(S4, [0], axis=0, out_shape=[1, 4, 4, 8]),
                                "job batching: GATHER with an activation params gathered along the batch axis"),
    "gather_constant_params_axis1": (lambda: G.raw_gather((4, 8), [[1, 2]], axis=1, const_params=True,
                                                          runtime_indices=True),
                                     "job batching: GATHER with constant params gathered along an axis other than 0"),
    "pack_axis0": (lambda: G.raw_pack(1, (4, 8), 0), "job batching: PACK on the batch axis"),
    "unpack_axis0": (lambda: G.raw_unpack((1, 4, 8), 0), "UNPACK does not keep the whole batch axis"),
    "tile_axis0": (lambda: G.raw_tile((1, 4), (2, 1)), "TILE does not keep the whole batch axis"),
    # accepted
    "gather_activation_constant_indices": (lambda: G.raw_gather(S4, [3, 0, 3], axis=2), None),
    "pack_axis1": (lambda: G.raw_pack(1, (1, 4, 8), 1), None),
    "unpack_axis1": (lambda: G.raw_unpack((1, 2, 4, 8), 1), None),
    "tile_inner": (lambda: G.raw_tile((1, 3, 4), (1, 2, 2)), None),
}


@pytest.mark.parametrize("name", sorted(BATCH_RULES))
def test_job_batch_rule(name):
    build, refusal = BATCH_RULES[name]
    buf = build()
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, 0)
    st = ex.PrepareJobBatches(m, key, 3)
    if refusal:
        assert not st.ok() and refusal in st.message(), st.message()
        assert ex.MaxJobBatch(key) == 1
        return
    assert st.ok(), st.message()
    assert ex.MaxJobBatch(key) == 3
    t_in = ex.GetInputs(key)[0]
    shape = read(buf)["tensors"][t_in]["shape"]
    xs = [G.fill(shape, np.int8) + np.int8(s) for s in range(3)]
    for s, x in enumerate(xs):
        ex.GetJobSlotView(key, t_in, 3, s).GetData()[...] = x
    assert ex.ExecuteJobBatch(key, 3).ok()
    for s, x in enumerate(xs):
        ref = run_reference(buf, x, table=REF_TABLE)
        for t in ex.GetOutputs(key):
            np.testing.assert_array_equal(ex.GetJobSlotView(key, t, 3, s).GetData().reshape(ref[t].shape), ref[t])


# ---- the synthesiser -------------------------------------------------------------------------
def test_existing_builders_write_the_same_bytes():
    """sha256 of three models, recorded on the parent commit"""
    assert hashlib.sha256(vit_tiny()).hexdigest() == "895af68c210b3409ad6d9875f754ab327c7b75c19d92067c2fa07bca1c30b0d4"
    assert hashlib.sha256(attention_block()).hexdigest() == \
        "3f35bd458a8d02ee0ab721205715f5c8f28a5e85c1df397fc6a274da0c63a232"
    assert hashlib.sha256(encoder_block(np.float32)).hexdigest() == \
        "0dc98cd831d52ff7b7fa340748fc8508d52fde48678d42698b8dd13ed0bf2358"


def test_text_encoder_parses_and_has_the_stated_graph():
    buf = text_encoder()
    om = OModel(buf)
    ops = [o.builtin for o in om.operators]
    assert ops[0] == G.GATHER and ops[1] == 0 and ops.count(G.GATHER) == 1  # GATHER, ADD
    assert ops[-2:] == [45, 9]  # STRIDED_SLICE, FULLY_CONNECTED
    ids = om.tensors[om.inputs[0]]
    assert ids.shape == [1, 128] and ids.np_dtype == np.int32
    table = om.tensors[om.operators[0].inputs[0]]
    assert table.is_const and table.shape == [1000, 192] and table.np_dtype == np.int8
    assert om.tensors[om.outputs[0]].shape == [1, 2]
    assert ops.count(40) == 2 * 5  # MEAN: two per LayerNorm, one LayerNorm up front and two per block
    for dtype, hybrid, want in ((np.float32, None, np.float32), (np.float32, "symmetric", np.float32)):
        om = OModel(text_encoder(dtype, hybrid=hybrid, **G.SMALL))
        table = om.tensors[om.operators[[o.builtin for o in om.operators].index(G.GATHER)].inputs[0]]
        assert table.is_const and table.np_dtype == want
    # the reader's option tables know the four unions, and the fields survive
    for name in ("GatherOptions", "TileOptions", "PackOptions", "UnpackOptions"):
        assert OPT[name] in OPTION_FIELDS, name
    seen = {(o["builtin"], o["options_type"]) for o in read(G.pack_unpack_tile())["ops"] if o["builtin"] in G.OPS}
    assert seen == {(G.GATHER, 23), (G.TILE, 51), (G.PACK, 59), (G.UNPACK, 64)}
