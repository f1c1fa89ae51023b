"""The re-indexing ops without a GPU: the references themselves, CpuReindex
through the C ABI on every launcher case, ReindexArgs' refusals and numpy
semantics through the kCPU executor, the model zoo, the job-batch rule and the
Python reader's option tables.  The reference is numpy (tests/reindex_models.py);
integer tensors are compared with assert_array_equal, float tensors at the
tolerance of tests/test_float_cpu.py."""
import ctypes

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi
from band_amd.tflite_reader_py import OPTION_FIELDS, read
from band_amd.tflite_synth import OPT, ModelBuilder, Table, int8_from_uint8
from tests import reindex_models as R
from tests.graph_reference import run_reference
from tests.test_float_cpu import assert_float_close


def _model(buf, mid=0):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    return m


def _differ(a, b):
    assert a.shape == b.shape
    return float((a != b).mean())


# ---- the references can tell mistakes apart ------------------------------------
@pytest.mark.parametrize("dtype", R.DTYPES)
def test_references_tell_wrong_variants_apart(dtype):
    """each wrong variant differs from the reference on >= 25 % of the elements
    of the fill (measured: the smallest share over all of them is 0.50).
    (3,2,1,0) and (1,0,2,3) are their own inverses - there the inverse
    permutation is no mistake - so for those the wrong variant is the
    untransposed tensor."""
    shares = []
    x = R.fill((4, 4, 4, 4), dtype)
    for perm in ((0, 3, 1, 2), (0, 2, 3, 1), (3, 2, 1, 0), (1, 0, 2, 3), (2, 0, 3, 1)):
        inverse = tuple(int(v) for v in np.argsort(perm))
        wrong = x if inverse == perm else np.transpose(x, inverse)
        shares.append(_differ(R.transpose_ref(x, perm), wrong))
    x = R.fill((2, 3, 5, 8), dtype)
    n, h, w, c = x.shape
    crd = x.reshape(n, h, w, 2, 2, 2).transpose(0, 1, 4, 2, 5, 3).reshape(n, h * 2, w * 2, 2)  # channel = c' 4 + by 2 + bx
    shares.append(_differ(R.depth_to_space_ref(x, 2), crd))
    swapped = x.reshape(n, h, w, 2, 2, 2).transpose(0, 1, 4, 2, 3, 5).reshape(n, h * 2, w * 2, 2)  # (bx, by)
    shares.append(_differ(R.depth_to_space_ref(x, 2), swapped))
    y = R.fill((2, 6, 10, 2), dtype)
    swapped = y.reshape(2, 3, 2, 5, 2, 2).transpose(0, 1, 3, 4, 2, 5).reshape(2, 3, 5, 8)
    shares.append(_differ(R.space_to_depth_ref(y, 2), swapped))
    np.testing.assert_array_equal(R.space_to_depth_ref(R.depth_to_space_ref(x, 2), 2), x)  # inverses
    z = R.fill((2, 9, 11, 6), dtype)
    ref = z[:, 7:1:-2, 1:10:3, ::-1]
    np.testing.assert_array_equal(
        R.strided_slice_ref(z, [0, 7, 1, 0], [0, 1, 10, 0], [1, -2, 3, -1], begin_mask=0b1001, end_mask=0b1001), ref)
    shares.append(_differ(ref, z[:, 7:1:-2, 1:10:3, :]))       # a dropped negative stride
    shares.append(_differ(ref, z[:, 6:0:-2, 1:10:3, ::-1]))    # a begin off by one
    shares.append(_differ(ref, z[:, 7:1:-2, 2:11:3, ::-1]))    # a slice start off by one
    assert min(shares) >= 0.25, shares
    print("smallest differing share:", min(shares))


# ---- CpuReindex through the C ABI ------------------------------------------------
CASES = [(name, dt, shape, view, kernel, mis) for name, dts, shape, view, kernel, mis in R.launcher_cases()
         for dt in dts]


@pytest.mark.parametrize("name,dtype,shape,view,kernel,misalign", CASES,
                         ids=["%s-%s" % (c[0], np.dtype(c[1]).name) for c in CASES])
def test_cpu_reindex_launcher_cases(name, dtype, shape, view, kernel, misalign):
    lib = _abi.load()
    x = R.fill(shape, dtype)
    v = view(x)
    want = np.ascontiguousarray(v)
    out = np.full(want.nbytes + 16, 0xff, np.uint8)
    p = R.reindex_params(x, v, x.ctypes.data, out.ctypes.data)
    assert lib.bhx_cpu_reindex(ctypes.byref(p)) == 0, lib.bhx_last_error()
    np.testing.assert_array_equal(out[:want.nbytes].view(dtype).reshape(want.shape), want)
    assert (out[want.nbytes:] == 0xff).all()
    if kernel is not None:  # the path is a pure function of the map: known without a device
        assert lib.bh_reindex_kernel(ctypes.byref(p)).decode() == kernel


def test_canonical_map():
    """unit dims go, mergeable dims merge, the identity is rank 1 stride 1"""
    lib = _abi.load()

    def canon(x, v):
        p, c = R.reindex_params(x, v, 0, 0), _abi.ReindexParams()
        assert lib.bh_reindex_canonical(ctypes.byref(p), ctypes.byref(c)) == 0
        return list(c.out_dims[:c.rank]), list(c.in_stride[:c.rank]), c.in_offset
    x = R.fill((2, 7, 7, 48), np.uint8)
    assert canon(x, x) == ([2 * 7 * 7 * 48], [1], 0)
    assert canon(x, x[..., 16:32]) == ([98, 16], [48, 1], 16)
    assert canon(x, x.transpose(0, 3, 1, 2)) == ([2, 48, 49], [49 * 48, 1, 48], 0)
    assert canon(x, x[:, :, :, ::-1]) == ([98, 48], [48, -1], 47)
    assert canon(x, x[::-1, ::-1, ::-1, ::-1]) == ([98 * 48], [-1], 98 * 48 - 1)
    p = _abi.ReindexParams(elem_bytes=1, rank=7)
    assert lib.bh_reindex_canonical(ctypes.byref(p), ctypes.byref(_abi.ReindexParams())) != 0
    assert lib.bh_reindex_kernel(ctypes.byref(p)) == b""
    assert lib.bhx_cpu_reindex(ctypes.byref(p)) != 0


# ---- raw one-op models -----------------------------------------------------------
def _raw(op, in_shape, out_shapes, consts=(), opt=None, opt_type=None, dtype=np.int8, out_scale=0.5,
         const_dtype=np.int32, runtime=None, x_pos=0):
    """x -> op -> outputs; consts become int tensors (index `runtime`: a model input instead)"""
    mb = ModelBuilder("raw")
    quant = np.dtype(dtype).itemsize == 1
    x = mb.tensor("x", list(in_shape), dtype, **(dict(scale=[0.5], zero_point=[3]) if quant else {}))
    mb.inputs.append(x)
    ins = []
    for i, c in enumerate(consts):
        a = np.asarray(c, const_dtype)
        if runtime == i:
            ins.append(mb.tensor("c%d" % i, list(a.shape), const_dtype))
            mb.inputs.append(ins[-1])
        else:
            ins.append(mb.tensor("c%d" % i, list(a.shape), const_dtype, data=a))
    ins.insert(x_pos, x)
    outs = [mb.tensor("y%d" % k, list(s), dtype, **(dict(scale=[out_scale], zero_point=[3]) if quant else {}))
            for k, s in enumerate(out_shapes)]
    mb.op(op, ins, outs, OPT[opt_type] if opt_type else 0, opt)
    mb.outputs += outs
    return mb.build()


def _ss_opt(begin_mask=0, end_mask=0, ellipsis=0, new_axis=0, shrink=0):
    return Table().set(0, "i", begin_mask).set(1, "i", end_mask).set(2, "i", ellipsis).set(3, "i", new_axis).set(
        4, "i", shrink)


def _n(v):
    return Table().set(0, "i", v)


S4 = (1, 4, 4, 8)
I4, O4 = [0, 0, 0, 0], [1, 1, 1, 1]
REFUSALS = {
    "runtime_perm": (lambda: _raw("TRANSPOSE", S4, [(1, 8, 4, 4)], [[0, 3, 1, 2]], Table(), "TransposeOptions",
                                  runtime=0), "TRANSPOSE perm must be a constant"),
    "runtime_begin": (lambda: _raw("SLICE", S4, [S4], [I4, list(S4)], Table(), "SliceOptions", runtime=0),
                      "SLICE begin / size must be constant"),
    "runtime_strides": (lambda: _raw("STRIDED_SLICE", S4, [S4], [I4, list(S4), O4], _ss_opt(), "StridedSliceOptions",
                                     runtime=2), "STRIDED_SLICE begin / end / strides must be constant"),
    "runtime_size_splits": (lambda: _raw("SPLIT_V", S4, [(1, 4, 4, 3), (1, 4, 4, 5)], [[3, 5], 3], _n(2),
                                         "SplitVOptions", runtime=0), "SPLIT_V size_splits must be a constant"),
    "runtime_axis": (lambda: _raw("SPLIT", S4, [(1, 4, 4, 4)] * 2, [3], _n(2), "SplitOptions", runtime=0, x_pos=1),
                     "SPLIT axis must be one constant"),
    "transpose_rank6": (lambda: _raw("TRANSPOSE", (1, 2, 2, 2, 2, 2), [(1, 2, 2, 2, 2, 2)], [[0, 1, 2, 3, 5, 4]],
                                     Table(), "TransposeOptions"), "TRANSPOSE rank > 5"),
    "slice_rank6": (lambda: _raw("SLICE", (1, 2, 2, 2, 2, 2), [(1, 2, 2, 2, 2, 1)], [[0] * 6, [1, 2, 2, 2, 2, 1]],
                                 Table(), "SliceOptions"), "SLICE rank > 5"),
    "strided_slice_rank6": (lambda: _raw("STRIDED_SLICE", (1, 2, 2, 2, 2, 2), [(1, 2, 2, 2, 2, 1)],
                                         [[0] * 6, [1, 2, 2, 2, 2, 1], [1] * 6], _ss_opt(), "StridedSliceOptions"),
                            "STRIDED_SLICE rank > 5"),
    "space_to_depth_rank3": (lambda: _raw("SPACE_TO_DEPTH", (4, 4, 4), [(2, 2, 16)], [], _n(2), "SpaceToDepthOptions"),
                             "SPACE_TO_DEPTH needs 4-D"),
    "depth_to_space_rank5": (lambda: _raw("DEPTH_TO_SPACE", (1, 1, 2, 2, 8), [(1, 1, 4, 4, 2)], [], _n(2),
                                          "DepthToSpaceOptions"), "DEPTH_TO_SPACE needs 4-D"),
    "not_a_permutation": (lambda: _raw("TRANSPOSE", S4, [(1, 4, 4, 8)], [[0, 1, 1, 3]], Table(), "TransposeOptions"),
                          "TRANSPOSE perm is not a permutation"),
    "stride_0": (lambda: _raw("STRIDED_SLICE", S4, [S4], [I4, list(S4), [1, 1, 0, 1]], _ss_opt(),
                              "StridedSliceOptions"), "STRIDED_SLICE stride 0"),
    "ellipsis_mask": (lambda: _raw("STRIDED_SLICE", S4, [S4], [I4, list(S4), O4], _ss_opt(ellipsis=2),
                                   "StridedSliceOptions"), "ellipsis_mask / new_axis_mask unsupported"),
    "new_axis_mask": (lambda: _raw("STRIDED_SLICE", S4, [S4], [I4, list(S4), O4], _ss_opt(new_axis=1),
                                   "StridedSliceOptions"), "ellipsis_mask / new_axis_mask unsupported"),
    "d2s_block": (lambda: _raw("DEPTH_TO_SPACE", (1, 4, 4, 6), [(1, 8, 8, 1)], [], _n(2), "DepthToSpaceOptions"),
                  "DEPTH_TO_SPACE block_size does not divide"),
    "s2d_block": (lambda: _raw("SPACE_TO_DEPTH", (1, 5, 4, 2), [(1, 2, 2, 8)], [], _n(2), "SpaceToDepthOptions"),
                  "SPACE_TO_DEPTH block_size does not divide"),
    "split_parts": (lambda: _raw("SPLIT", S4, [(1, 4, 4, 2)] * 3, [3], _n(3), "SplitOptions", x_pos=1),
                    "SPLIT axis extent is not a multiple"),
    "split_v_sum": (lambda: _raw("SPLIT_V", S4, [(1, 4, 4, 3), (1, 4, 4, 4)], [[3, 4], 3], _n(2), "SplitVOptions"),
                    "SPLIT_V size_splits do not sum"),
    "split_v_two_open": (lambda: _raw("SPLIT_V", S4, [(1, 4, 4, 4)] * 2, [[-1, -1], 3], _n(2), "SplitVOptions"),
                         "SPLIT_V size_splits do not sum"),
    "quantization": (lambda: _raw("TRANSPOSE", S4, [(1, 8, 4, 4)], [[0, 3, 1, 2]], Table(), "TransposeOptions",
                                  out_scale=0.25), "output quantization differs from the input's"),
    "shape_disagrees": (lambda: _raw("SLICE", S4, [(1, 2, 3, 8)], [[0, 1, 1, 0], [1, 2, 2, 8]], Table(),
                                     "SliceOptions"), "output shape differs"),
    "slice_outside": (lambda: _raw("SLICE", S4, [(1, 2, 2, 8)], [[0, 3, 1, 0], [1, 2, 2, 8]], Table(), "SliceOptions"),
                      "SLICE begin / size outside the input"),
    "element_type": (lambda: _raw("TRANSPOSE", S4, [(1, 8, 4, 4)], [[0, 3, 1, 2]], Table(), "TransposeOptions",
                                  dtype=np.float16), "element type must be int8, uint8, float32 or int32"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_say_why(name):
    """the op is in unsupported_ops of every worker, and the lowering error names the reason"""
    build, reason = REFUSALS[name]
    m = _model(build())
    spec = HipModelExecutor(0, 0, DeviceFlag.kCPU).InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kCPU] == {0}
    st = HipModelExecutor(0, 0, DeviceFlag.kCPU).PrepareSubgraph(m)
    assert not st.ok() and reason in st.message(), st.message()


def test_refuses_an_output_without_elements():
    """x[:, 3:3] is empty: unsupported (a zero-byte tensor cannot even get a mirror, so only the set says so)"""
    m = _model(_raw("STRIDED_SLICE", S4, [(1, 0, 4, 8)], [[0, 3, 0, 0], [1, 3, 4, 8], O4], _ss_opt(),
                    "StridedSliceOptions"))
    assert HipModelExecutor(0, 0, DeviceFlag.kCPU).InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kCPU] == {0}
    assert not HipModelExecutor(0, 0, DeviceFlag.kCPU).PrepareSubgraph(m).ok()


def _run_raw(buf, x, flag=DeviceFlag.kCPU, worker=0):
    m = _model(buf)
    ex = HipModelExecutor(0, worker, flag)
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, worker)
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = x
    assert ex.ExecuteSubgraph(key).ok()
    return [ex.GetTensorView(key, t).GetData().copy() for t in ex.GetOutputs(key)]


SS = (2, 9, 11, 6)
STRIDED = [  # begin, end, strides, begin_mask, end_mask, shrink_axis_mask
    ([0, 7, 1, 0], [0, 1, 10, 0], [1, -2, 3, -1], 0b1001, 0b1001, 0),   # x[:, 7:1:-2, 1:10:3, ::-1]
    ([0, -100, 50, 2], [2, 100, -100, 100], [1, 1, -1, 2], 0, 0, 0),    # out-of-range bounds clamp
    ([-1, -3, -5, -2], [-3, -1, -1, -1], [-1, 1, 2, 1], 0, 0, 0),       # negative indices
    ([1, 2, 3, 4], [0, 0, 0, 0], [1, 1, 1, 1], 0, 0b0110, 0b1001),      # x[1, 2:, 3:, 4]
    ([0, -1, 0, 0], [0, 0, 0, 0], [1, 1, 1, 1], 0b1101, 0b1101, 0b0010),  # x[:, -1]
    ([1, 8, 10, 5], [0, 0, 0, 0], [-1, -3, -4, -5], 0, 0b1111, 0),      # negative strides to the start
    ([0, 0, 0, 0], [2, 9, 11, 6], [1, 1, 1, 1], 0, 0, 0),               # everything: a copy
    ([0, 0, 0, 5], [0, 0, 0, 0], [1, 1, 1, 1], 0b0100, 0b0100, 0b1011),  # x[0, 0, :, 5]
]


@pytest.mark.parametrize("case", range(len(STRIDED)))
@pytest.mark.parametrize("dtype", [np.int8, np.float32])
def test_strided_slice_is_numpy_indexing(case, dtype):
    begin, end, strides, bm, em, sm = STRIDED[case]
    x = R.fill(SS, dtype)
    want = R.strided_slice_ref(x, begin, end, strides, bm, em, sm)
    assert want.size > 0
    buf = _raw("STRIDED_SLICE", SS, [want.shape], [begin, end, strides], _ss_opt(bm, em, shrink=sm),
               "StridedSliceOptions", dtype=dtype)
    got, = _run_raw(buf, x)
    assert got.dtype == dtype
    np.testing.assert_array_equal(got.reshape(want.shape), want)


@pytest.mark.parametrize("const_dtype", [np.int32, np.int64])
def test_one_op_models_on_cpu_executor(const_dtype):
    """each op alone, index tensors int32 and int64, against numpy"""
    x = R.fill((2, 6, 4, 12), np.uint8)
    cases = [
        ("TRANSPOSE", [[3, 0, 2, 1]], Table(), "TransposeOptions", 0, [R.transpose_ref(x, (3, 0, 2, 1))]),
        ("SLICE", [[1, 2, 0, 3], [-1, 3, 4, 5]], Table(), "SliceOptions", 0, [R.slice_ref(x, [1, 2, 0, 3], [-1, 3, 4, 5])]),
        ("SPLIT", [-1], _n(3), "SplitOptions", 1, R.split_ref(x, 3, -1)),
        ("SPLIT", [1], _n(2), "SplitOptions", 1, R.split_ref(x, 2, 1)),
        ("SPLIT_V", [[5, -1, 3], -1], _n(3), "SplitVOptions", 0, R.split_v_ref(x, [5, -1, 3], 3)),
        ("SPLIT_V", [[1, 1], 0], _n(2), "SplitVOptions", 0, R.split_v_ref(x, [1, 1], 0)),
        ("DEPTH_TO_SPACE", [], _n(2), "DepthToSpaceOptions", 0, [R.depth_to_space_ref(x, 2)]),
        ("SPACE_TO_DEPTH", [], _n(2), "SpaceToDepthOptions", 0, [R.space_to_depth_ref(x, 2)]),
    ]
    for op, consts, opt, opt_type, x_pos, want in cases:
        buf = _raw(op, x.shape, [w.shape for w in want], consts, opt, opt_type, dtype=np.uint8,
                   const_dtype=const_dtype, x_pos=x_pos)
        got = _run_raw(buf, x)
        assert len(got) == len(want)
        for g, w in zip(got, want):
            np.testing.assert_array_equal(g.reshape(w.shape), w, err_msg=op)


# ---- the zoo -----------------------------------------------------------------------
def _compare(name, t, got, ref):
    assert got.dtype == ref.dtype, (name, t)
    if ref.dtype == np.float32:
        assert_float_close(got, ref, "%s tensor %d" % (name, t))
    else:
        np.testing.assert_array_equal(got.reshape(ref.shape), ref, err_msg="%s tensor %d" % (name, t))


def non_constant_tensors(buf):
    return [i for i, t in enumerate(read(buf)["tensors"]) if t["data"] is None]


@pytest.fixture(scope="module")
def zoo_refs():
    out = {}
    for name, build in R.ZOO.items():
        buf = build()
        x = R.zoo_input(buf, seed=3)
        out[name] = (buf, x, run_reference(buf, x))
    return out


@pytest.mark.parametrize("name", sorted(R.ZOO))
def test_zoo_on_cpu_executor_every_tensor(zoo_refs, name):
    buf, x, ref = zoo_refs[name]
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kCPU] == set()
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, 0)
    views = {t: ex.GetTensorView(key, t) for t in non_constant_tensors(buf)}
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = x
    assert ex.ExecuteSubgraph(key).ok()
    assert any(o["builtin"] in R.REINDEX_OPS for o in read(buf)["ops"])
    for t, v in views.items():
        _compare(name, t, v.GetData(), ref[t])


def test_zoo_inputs_reach_the_reindex_ops(zoo_refs):
    """the tensors the re-indexing ops move are not constant: a wrong map would show"""
    for name, (buf, x, ref) in zoo_refs.items():
        for o in read(buf)["ops"]:
            if o["builtin"] in R.REINDEX_OPS:
                for t in o["outputs"]:
                    assert len(np.unique(ref[t])) > min(8, ref[t].size // 4), (name, t)


# ---- job batching ------------------------------------------------------------------
@pytest.mark.parametrize("name", ["shuffle_unit", "detector_head_i8", "subpixel"])
def test_job_batch_of_3_on_cpu(name):
    buf = R.ZOO[name]()
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(0, 0)
    st = ex.PrepareJobBatches(m, key, 3)
    assert st.ok(), st.message()
    xs = [R.zoo_input(buf, seed=10 + s) for s in range(3)]
    for s, x in enumerate(xs):
        ex.GetJobSlotView(key, ex.GetInputs(key)[0], 3, s).GetData()[...] = x
    assert ex.ExecuteJobBatch(key, 3).ok()
    for s, x in enumerate(xs):
        ref = run_reference(buf, x)
        for t in ex.GetOutputs(key):
            _compare(name, t, ex.GetJobSlotView(key, t, 3, s).GetData().reshape(ref[t].shape), ref[t])


BATCH_RULES = {
    # refused: the map touches axis 0 other than as the full range
    "transpose_batch": (R.batch_axis_transpose, "TRANSPOSE does not keep the whole batch axis"),
    "split_axis0": (lambda: _raw("SPLIT", S4, [S4], [0], _n(1), "SplitOptions", x_pos=1),
                    "SPLIT does not keep the whole batch axis"),
    "split_v_axis0": (lambda: _raw("SPLIT_V", S4, [S4], [[1], 0], _n(1), "SplitVOptions"),
                      "SPLIT_V does not keep the whole batch axis"),
    "slice_part_of_axis0": (lambda: _raw("SLICE", (2, 4, 4, 8), [S4], [[1, 0, 0, 0], [1, 4, 4, 8]], Table(),
                                         "SliceOptions"), "SLICE does not keep the whole batch axis"),
    "strided_slice_shrinks_axis0": (lambda: _raw("STRIDED_SLICE", S4, [(4, 4, 8)], [I4, list(S4), O4],
                                                 _ss_opt(shrink=1), "StridedSliceOptions"),
                                    "STRIDED_SLICE does not keep the whole batch axis"),
    "strided_slice_reverses_axis0": (lambda: _raw("STRIDED_SLICE", S4, [S4], [I4, list(S4), [-1, 1, 1, 1]],
                                                  _ss_opt(0b0001, 0b0001), "StridedSliceOptions"),
                                     "STRIDED_SLICE does not keep the whole batch axis"),
    # accepted: begin 0, end 1, stride 1 on a unit batch is the whole axis; so is size 1 from 0
    "strided_slice_0_to_1": (lambda: _raw("STRIDED_SLICE", S4, [(1, 2, 4, 8)], [[0, 1, 0, 0], [1, 3, 4, 8], O4],
                                          _ss_opt(), "StridedSliceOptions"), None),
    "slice_size_1": (lambda: _raw("SLICE", S4, [(1, 2, 4, 8)], [[0, 2, 0, 0], [1, 2, 4, 8]], Table(), "SliceOptions"),
                     None),
    "transpose_keeps_batch": (lambda: _raw("TRANSPOSE", S4, [(1, 8, 4, 4)], [[0, 3, 1, 2]], Table(),
                                           "TransposeOptions"), None),
    "split_channels": (lambda: _raw("SPLIT", S4, [(1, 4, 4, 4)] * 2, [3], _n(2), "SplitOptions", x_pos=1), None),
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
    t_in, t_out = ex.GetInputs(key)[0], ex.GetOutputs(key)[0]
    shape = read(buf)["tensors"][t_in]["shape"]
    xs = [R.fill(shape, np.int8) + np.int8(s) for s in range(3)]
    for s, x in enumerate(xs):
        ex.GetJobSlotView(key, t_in, 3, s).GetData()[...] = x
    assert ex.ExecuteJobBatch(key, 3).ok()
    for s, x in enumerate(xs):
        ref = run_reference(buf, x)[t_out]
        np.testing.assert_array_equal(ex.GetJobSlotView(key, t_out, 3, s).GetData().reshape(ref.shape), ref)


def test_batch_axis_transpose_still_runs():
    buf = R.batch_axis_transpose()
    x = R.zoo_input(buf, seed=1)
    ref = run_reference(buf, x)
    got, = _run_raw(buf, x)
    t = read(buf)["outputs"][0]
    np.testing.assert_array_equal(got.reshape(ref[t].shape), ref[t])


# ---- the Python reader ---------------------------------------------------------------
def test_python_reader_round_trips_the_option_tables():
    """the synthesiser's union numbers are the reader table's keys, every option
    field survives read(), and a model rewritten from what read() returns
    (int8_from_uint8) still resolves to the same maps"""
    for name in ("TransposeOptions", "StridedSliceOptions", "SplitOptions", "SliceOptions", "SplitVOptions",
                 "SpaceToDepthOptions", "DepthToSpaceOptions"):
        assert OPT[name] in OPTION_FIELDS, name
    seen = set()
    for build in list(R.ZOO.values()) + [R.batch_axis_transpose]:
        for o in read(build())["ops"]:
            if o["builtin"] in R.REINDEX_OPS:
                assert o["options_type"] != 0 and o["options"] is not None
                seen.add((o["builtin"], o["options_type"]))
    assert seen == {(R.TRANSPOSE, 26), (R.STRIDED_SLICE, 32), (R.SPLIT, 35), (R.SLICE, 44), (R.SPLIT_V, 79),
                    (R.SPACE_TO_DEPTH, 19), (R.DEPTH_TO_SPACE, 94)}
    cls = [o for o in read(R.detector_head(np.uint8))["ops"] if o["builtin"] == R.STRIDED_SLICE][2]
    fields = {slot: v for slot, (_, v) in cls["options"].fields.items()}
    assert fields.get(0, 0) == 15 and fields.get(1, 0) == 31 and fields.get(4, 0) == 0
    sub = [o for o in read(R.subpixel())["ops"] if o["builtin"] in (R.SPACE_TO_DEPTH, R.DEPTH_TO_SPACE)]
    assert [o["options"].fields[0][1] for o in sub] == [2, 2]
    split = [o for o in read(R.shuffle_unit())["ops"] if o["builtin"] == R.SPLIT][0]
    assert split["options"].fields[0][1] == 2 and len(split["outputs"]) == 2
    # rewritten through the reader: the uint8 detector head as int8
    buf = int8_from_uint8(R.detector_head(np.uint8))
    x = R.zoo_input(buf, seed=5)
    ref = run_reference(buf, x)
    got = _run_raw(buf, x)
    for t, g in zip(read(buf)["outputs"], got):
        np.testing.assert_array_equal(g.reshape(ref[t].shape), ref[t])
