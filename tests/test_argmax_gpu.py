"""ARG_MAX / ARG_MIN on the MI355X: the bh_argminmax launcher (thread-per-row,
strided and wave-per-row forms), the fused bh_resize_bilinear_argminmax_i8
launcher, and whole models through the executor and the engine.

Reference: tests.argmax_models.arg_ref (the restated sequential loop of
reference_ops::ArgMinMax) over the input, over oracle.runner.resize_bilinear_i8
for the fused launcher, and over the oracle's run of the model's twin without
the tails for models.  Everything is assert_array_equal."""
import ctypes

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
from band_amd.tflite_reader_py import read
from band_amd.tflite_synth import deeplab_v3_mobilenet_v2
from oracle import runner as orc
from tests.argmax_models import (arg_ref, argmax_zoo, argmax_zoo_ref, deeplab_logits, tied_pixels)

pytestmark = pytest.mark.gpu

DTYPES = {"i8": (np.int8, 0), "u8": (np.uint8, 1), "f32": (np.float32, 2)}


def _dev(a):
    from band_amd.device import DeviceBuffer
    return DeviceBuffer.from_array(np.ascontiguousarray(a))


def _argminmax(lib, x3, in_type, minimum, out, offset=0):
    """bh_argminmax over x3 [outer][axis_len][inner], uploaded `offset` bytes into its buffer"""
    from band_amd import _abi
    from band_amd.device import DeviceBuffer
    outer, length, inner = x3.shape
    raw = np.concatenate([np.zeros(offset, np.uint8), np.ascontiguousarray(x3).view(np.uint8).reshape(-1)])
    dx = _dev(raw)
    ob = np.dtype(out).itemsize
    dy = _dev(np.full(outer * inner * ob, 0xff, np.uint8))  # stale bytes: a missing high word would show
    p = _abi.ArgMinMaxParams(outer=outer, axis_len=length, inner=inner, in_type=in_type, is_min=int(minimum),
                             out_bytes=ob, input=dx.value + offset, output=dy.value)
    _abi.check(lib.bh_argminmax(ctypes.byref(p), None), "bh_argminmax")
    got = dy.download(out, (outer, inner))
    if ob == 8:
        assert (got.view(np.uint32).reshape(outer, inner, 2)[..., 1] == 0).all(), "int64 high words"
    return got, lib.bh_argminmax_kernel(ctypes.byref(p)).decode()


def _random(rng, shape, dtype):
    """a narrow range of values, so most rows hold their extreme several times"""
    if dtype == np.float32:
        return (rng.integers(-3, 4, shape) * 0.5).astype(np.float32)
    mid = 0 if dtype == np.int8 else 128
    return rng.integers(mid - 3, mid + 4, shape).astype(dtype)


SHAPES = [(1, 1, 1), (7, 21, 1), (3, 5, 11), (300, 2, 1), (5, 64, 1), (5, 65, 1), (3, 257, 1), (2, 1001, 1),
          (1, 21, 3136)]


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("shape", SHAPES)
def test_argminmax_launcher(gpu_lib, shape, dt):
    dtype, code = DTYPES[dt]
    rng = np.random.default_rng(sum(shape) + code)
    narrow = _random(rng, shape, dtype)
    wide = (rng.standard_normal(shape).astype(np.float32) if dtype == np.float32
            else rng.integers(np.iinfo(dtype).min, np.iinfo(dtype).max + 1, shape).astype(dtype))
    for x in (narrow, wide):
        for minimum in (False, True):
            for out in (np.int32, np.int64):
                got, kernel = _argminmax(gpu_lib, x, code, minimum, out)
                np.testing.assert_array_equal(got, arg_ref(x, 1, minimum, out), err_msg="%s min=%d" % (kernel, minimum))
                assert kernel == ("argminmax_row_kernel" if shape[2] == 1 and shape[1] >= 64 else "argminmax_kernel")


def _directed_rows(dtype, length):
    """rows of `length` whose answer a wrong rule gets wrong (extremes placed for ARG_MAX and ARG_MIN)"""
    if dtype == np.float32:
        lo, hi, base = -5.0, 5.0, 1.0
    elif dtype == np.int8:
        lo, hi, base = -128, 127, 3
    else:
        lo, hi, base = 0, 255, 0x7f
    rows = []

    def row(fill=base):
        return np.full(length, fill, dtype)
    rows.append(row())                           # all equal: index 0
    r = row(); r[-1] = hi; rows.append(r)        # maximum at the last element
    r = row(); r[-1] = lo; rows.append(r)        # minimum at the last element
    r = row(); r[0] = r[-1] = hi; rows.append(r)  # the extreme at both ends: the lower index
    r = row(); r[0] = r[-1] = lo; rows.append(r)
    if length > 2:
        r = row(); r[1] = r[-1] = hi; r[length // 2] = hi; rows.append(r)
        r = row(); r[1] = r[-1] = lo; r[length // 2] = lo; rows.append(r)
    if dtype == np.uint8 and length > 2:         # a signed read would order these the other way
        r = row(0x7f); r[length // 2] = 0x80; rows.append(r)
        r = row(0x80); r[length // 2] = 0x7f; rows.append(r)
        r = row(0x7f); r[-1] = 0x80; r[1] = 0x80; rows.append(r)
    if dtype == np.float32 and length > 4:
        nan, inf = np.float32(np.nan), np.float32(np.inf)
        r = row(); r[0] = nan; r[3] = 9.0; r[4] = -9.0; rows.append(r)        # NaN first: 0 for both ops
        r = row(); r[length // 2] = nan; r[-1] = 2.0; r[-2] = -2.0; rows.append(r)  # NaN in the middle: skipped
        r = row(); r[1] = nan; r[2] = nan; rows.append(r)                      # ... among equals: 0
        r = row(); r[2] = inf; r[-1] = inf; r[3] = -inf; r[-2] = -inf; rows.append(r)
        r = row(-inf); rows.append(r)                                          # all -inf: 0
        r = row(inf); r[length // 2] = nan; rows.append(r)
        r = row(0.0); r[0] = -0.0; r[-1] = 0.0; rows.append(r)                 # -0.0 == +0.0: 0
        r = row(0.0); r[1::2] = -0.0; rows.append(r)
        r = row(-1.0); r[2] = -0.0; r[4] = 0.0; rows.append(r)
        r = row(1.0); r[2] = 0.0; r[4] = -0.0; rows.append(r)
    return np.stack(rows)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("length", [2, 21, 64, 65, 1001])
def test_argminmax_directed(gpu_lib, length, dt):
    """all-equal rows, the extreme at the last element and at both ends (the
    cross-lane reduction must prefer the lower index), 0x7f / 0x80, NaN first
    and in the middle, +-inf, -0.0 / +0.0 - as contiguous rows (inner 1) and
    as a middle axis (inner = the number of rows)"""
    dtype, code = DTYPES[dt]
    rows = _directed_rows(dtype, length)
    for x3 in (rows[:, :, None], np.ascontiguousarray(rows.T)[None]):
        for minimum in (False, True):
            for out in (np.int32, np.int64):
                got, kernel = _argminmax(gpu_lib, x3, code, minimum, out)
                np.testing.assert_array_equal(got, arg_ref(x3, 1, minimum, out), err_msg="%s min=%d" % (kernel, minimum))
    ref = arg_ref(rows, 1)
    assert ref[0] == 0 and ref[1] == length - 1 and ref[3] == 0


@pytest.mark.parametrize("shape,offset", [((7, 21, 1), 1), ((7, 21, 1), 3), ((2, 1001, 1), 1), ((3, 5, 11), 2),
                                          ((9, 3, 1), 3)])
def test_argminmax_misaligned_input(gpu_lib, shape, offset):
    """8-bit input that starts off a dword boundary (the covering-dword reads
    of the row form, the byte reads of the others)"""
    rng = np.random.default_rng(offset + shape[1])
    for dtype, code in (DTYPES["i8"], DTYPES["u8"]):
        x = _random(rng, shape, dtype)
        for minimum in (False, True):
            got, _ = _argminmax(gpu_lib, x, code, minimum, np.int32, offset=offset)
            np.testing.assert_array_equal(got, arg_ref(x, 1, minimum))


def test_argminmax_refuses_bad_parameters(gpu_lib):
    from band_amd import _abi
    x, y = _dev(np.zeros(64, np.int8)), _dev(np.zeros(64, np.int8))
    for bad in (dict(outer=0), dict(in_type=3), dict(out_bytes=2), dict(output=y.value + 4, out_bytes=8)):
        kw = dict(outer=2, axis_len=4, inner=1, in_type=0, is_min=0, out_bytes=4, input=x.value, output=y.value)
        kw.update(bad)
        p = _abi.ArgMinMaxParams(**kw)
        assert gpu_lib.bh_argminmax(ctypes.byref(p), None) != 0
        assert b"bh_argminmax" in gpu_lib.bh_last_error()


# ---- the fused launcher ------------------------------------------------------
def _tab(n_in, n_out, ac, hp):
    """the executor's BilinearIntegerTable: lower row, upper row, 10-bit scaled coordinate"""
    s = ((1 << 10) * n_in + n_out // 2) // n_out
    if ac and n_out > 1:
        s = ((1 << 10) * (n_in - 1) + (n_out - 1) // 2) // (n_out - 1)
    t = []
    for v in range(n_out):
        sc = v * s + s // 2 - (1 << 9) if hp else v * s
        lo = max(int(np.trunc(sc / 1024)), 0)
        hi = min(int(np.trunc((sc + 1023) / 1024)), n_in - 1)
        t += [lo, hi, sc]
    return np.array(t, np.int32)


def _fused_params(x, oh, ow, ac, hp, minimum, out, keep):
    from band_amd import _abi
    b, ih, iw, c = x.shape
    dx, dty, dtx = _dev(x), _dev(_tab(ih, oh, ac, hp)), _dev(_tab(iw, ow, ac, hp))
    dy = _dev(np.full(b * oh * ow * np.dtype(out).itemsize, 0xff, np.uint8))
    keep += [dx, dty, dtx, dy]
    rz = _abi.ResizeBilinearParams(batch=b, in_h=ih, in_w=iw, channels=c, out_h=oh, out_w=ow, y_tab=dty.value,
                                   x_tab=dtx.value, input=dx.value, output=dy.value)
    return _abi.ResizeArgMinMaxParams(rz=rz, is_min=int(minimum), out_bytes=np.dtype(out).itemsize), dy


GEOMETRIES = [(2, 5, 7, 33, 47, c, ac, hp) for c in (1, 2, 16, 19, 21, 64) for ac, hp in ((1, 0), (0, 1))] + [
    (2, 14, 14, 30, 30, 21, 0, 0), (2, 9, 9, 4, 5, 19, 0, 1), (2, 6, 6, 6, 6, 16, 0, 0), (3, 5, 7, 33, 47, 21, 1, 0),
    # enough output rows for 2 and for 8 rows per workgroup, the last group partial
    (64, 3, 4, 37, 9, 5, 0, 1), (128, 3, 4, 61, 9, 5, 1, 0)]


@pytest.mark.parametrize("b,ih,iw,oh,ow,c,ac,hp", GEOMETRIES)
def test_resize_argminmax_launcher(gpu_lib, b, ih, iw, oh, ow, c, ac, hp):
    from band_amd import _abi
    rng = np.random.default_rng(100 * c + ow + ac)
    full = rng.integers(-128, 128, (b, ih, iw, c)).astype(np.int8)
    small = rng.integers(-6, 7, (b, ih, iw, c)).astype(np.int8)
    for x in (full, small):
        resized = orc.resize_bilinear_i8(x, (oh, ow), ac, hp)
        if (ih, iw, c) == (5, 7, 21) and x is full:  # the inputs exercise many indices ...
            assert len(np.unique(arg_ref(resized, 3))) >= 15
        if (b, ih, iw, oh, ow, c, hp) == (2, 5, 7, 33, 47, 21, 1) and x is small:  # ... and many ties
            assert tied_pixels(resized) >= 500
        for minimum in (False, True):
            for out in (np.int32, np.int64):
                keep = []
                p, dy = _fused_params(x, oh, ow, ac, hp, minimum, out, keep)
                assert gpu_lib.bh_resize_bilinear_argminmax_i8_ok(ctypes.byref(p)) == 0
                _abi.check(gpu_lib.bh_resize_bilinear_argminmax_i8(ctypes.byref(p), None), "fused")
                got = dy.download(out, (b, oh, ow))
                np.testing.assert_array_equal(got, arg_ref(resized, 3, minimum, out))
                if out == np.int64:
                    assert (got.view(np.uint32).reshape(b, oh, ow, 2)[..., 1] == 0).all()


def test_resize_argminmax_refuses_rows_too_large_for_lds(gpu_lib):
    """a blended input row of 300 x 65 words (78 KB) does not fit: nonzero, a
    message, no launch; so does a row of more than 1024 output columns"""
    keep = []
    x = np.zeros((1, 2, 300, 64), np.int8)
    p, _ = _fused_params(x, 4, 600, 0, 0, False, np.int32, keep)
    assert gpu_lib.bh_resize_bilinear_argminmax_i8_ok(ctypes.byref(p)) != 0
    assert gpu_lib.bh_resize_bilinear_argminmax_i8(ctypes.byref(p), None) != 0
    assert b"LDS" in gpu_lib.bh_last_error()
    p, _ = _fused_params(np.zeros((1, 2, 3, 2), np.int8), 4, 1030, 0, 0, False, np.int32, keep)
    assert gpu_lib.bh_resize_bilinear_argminmax_i8(ctypes.byref(p), None) != 0
    p, _ = _fused_params(np.zeros((1, 2, 3, 2), np.int8), 4, 8, 0, 0, False, np.int32, keep)
    p.out_bytes = 2
    assert gpu_lib.bh_resize_bilinear_argminmax_i8(ctypes.byref(p), None) != 0


# ---- models ------------------------------------------------------------------
SIZE = 64


@pytest.fixture(scope="module")
def deeplab_refs():
    """8 inputs of the size-64 model and the oracle's logits of the twin for each"""
    rng = np.random.default_rng(5)
    xs = [rng.integers(-128, 128, (1, SIZE, SIZE, 3)).astype(np.int8) for _ in range(8)]
    return xs, [deeplab_logits(SIZE, x) for x in xs]


def _exec(buf, mid=31):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(mid, 1, DeviceFlag.kGPU)
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    ex._model_ref = m
    return m, ex, SubgraphKey(mid, 1)


FOLDED, UNFOLDED = "resize_bilinear_argminmax_kernel", "argminmax_kernel"


@pytest.mark.parametrize("out", [np.int32, np.int64])
@pytest.mark.parametrize("fusion", [None, "noargmax", "0"])
def test_deeplab_argmax_executor(gpu_lib, monkeypatch, deeplab_refs, fusion, out):
    """the map equals the reference under the default lowering (one folded
    launch), BAND_HIP_FUSION=noargmax and =0 (resize + argminmax launches):
    eager pass, then the captured graph; then a view of the resized logits
    materialises them (the fold is undone) and both tensors are right"""
    if fusion is None:
        monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    else:
        monkeypatch.setenv("BAND_HIP_FUSION", fusion)
    xs, logits = deeplab_refs
    buf = deeplab_v3_mobilenet_v2(np.int8, size=SIZE, argmax=out)
    m, ex, key = _exec(buf)
    kernels = [r["kernel"] for r in ex.ProfileSubgraph(key, iters=1)]
    if fusion is None:
        assert FOLDED in kernels and UNFOLDED not in kernels, kernels
    else:
        assert UNFOLDED in kernels and FOLDED not in kernels and "resize_bilinear_kernel" in kernels, kernels
    t_in, t_out = ex.GetInputs(key)[0], ex.GetOutputs(key)[0]
    for i in (0, 1, 2):  # eager, then the captured graph twice
        ex.GetTensorView(key, t_in).GetData()[...] = xs[i]
        assert ex.ExecuteSubgraph(key).ok()
        got = ex.GetTensorView(key, t_out).GetData()
        assert got.dtype == out and got.shape == (1, SIZE, SIZE)
        np.testing.assert_array_equal(got, arg_ref(logits[i], 3, out=out))
    arg_op = [o for o in read(buf)["ops"] if o["builtin"] == 56][0]
    resized = ex.GetTensorView(key, arg_op["inputs"][0])
    assert resized is not None
    kernels = [r["kernel"] for r in ex.ProfileSubgraph(key, iters=1)]
    assert UNFOLDED in kernels and FOLDED not in kernels, kernels
    for i in (3, 4):
        ex.GetTensorView(key, t_in).GetData()[...] = xs[i]
        assert ex.ExecuteSubgraph(key).ok()
        np.testing.assert_array_equal(resized.GetData(), logits[i])
        np.testing.assert_array_equal(ex.GetTensorView(key, t_out).GetData(), arg_ref(logits[i], 3, out=out))


@pytest.mark.parametrize("out", [np.int32, np.int64])
def test_deeplab_argmax_job_batches(gpu_lib, monkeypatch, deeplab_refs, out):
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    xs, logits = deeplab_refs
    m, ex, key = _exec(deeplab_v3_mobilenet_v2(np.int8, size=SIZE, argmax=out), 32)
    st = ex.PrepareJobBatches(m, key, 8)
    assert st.ok(), st.message()
    t_in, t_out = ex.GetInputs(key)[0], ex.GetOutputs(key)[0]
    for n in (2, 3, 5, 8):
        order = [(s + n) % 8 for s in range(n)]
        for s, i in enumerate(order):
            ex.GetJobSlotView(key, t_in, n, s).GetData()[...] = xs[i]
        for _ in range(2):
            assert ex.ExecuteJobBatch(key, n).ok()
            for s, i in enumerate(order):
                got = ex.GetJobSlotView(key, t_out, n, s).GetData()
                np.testing.assert_array_equal(got.reshape(1, SIZE, SIZE), arg_ref(logits[i], 3, out=out),
                                              err_msg="n=%d slot %d" % (n, s))


def test_argmax_zoo_gpu_executor(gpu_lib, monkeypatch):
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    x = np.random.default_rng(7).integers(-128, 128, (1, 6, 5, 8)).astype(np.int8)
    ref = argmax_zoo_ref(x)
    m, ex, key = _exec(argmax_zoo(), 33)
    spec = ex.InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kGPU] == set()
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = x
    for _ in range(2):
        assert ex.ExecuteSubgraph(key).ok()
        outs = [ex.GetTensorView(key, t).GetData() for t in ex.GetOutputs(key)]
        assert len(outs) == len(ref)
        for g, r in zip(outs, ref):
            assert g.dtype == r.dtype
            np.testing.assert_array_equal(g.reshape(r.shape), r)


def test_engine_two_gpu_workers_batch_argmax_jobs(gpu_lib, tmp_path, monkeypatch, deeplab_refs):
    from band_amd.engine import Engine, JobStatus, Model, SchedulerType, make_config, kBandOk
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    xs, logits = deeplab_refs
    e = Engine(make_config([SchedulerType.kRoundRobin], [DeviceFlag.kGPU] * 2, max_job_batch=4))
    path = str(tmp_path / "deeplab_argmax.tflite")
    with open(path, "wb") as f:
        f.write(deeplab_v3_mobilenet_v2(np.int8, size=SIZE, argmax=np.int32))
    m = Model()
    assert m.FromPath(path)
    assert e.RegisterModel(m)
    assert e.GetNumOutputTensors(m) == 1
    prepared = []
    for i in range(24):
        t = e.CreateInputTensor(m, 0)
        t.data()[...] = xs[i % 8]
        prepared.append((i % 8, t, [e.CreateOutputTensor(m, 0)]))
    jobs = [(e.RequestAsync(m, [t]), i, outs) for i, t, outs in prepared]
    for h, i, outs in jobs:
        assert h >= 0 and e.Wait(h, outs) == kBandOk
        assert e.GetJobRecord(h).status == JobStatus.kSuccess
        got = outs[0].data()
        assert got.dtype == np.int32
        np.testing.assert_array_equal(got.reshape(1, SIZE, SIZE), arg_ref(logits[i], 3))
    e.close()
