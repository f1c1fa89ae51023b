"""Fixtures of the re-indexing ops (TRANSPOSE, STRIDED_SLICE, SLICE, SPLIT,
SPLIT_V, SPACE_TO_DEPTH, DEPTH_TO_SPACE): the numpy references, the fills, the
launcher cases, the model zoo and eval_reindex.

The reference is numpy and nothing else: every op copies elements, so parity
is exact.  The oracle does not know these ops; tests.graph_reference walks a
model op by op and evaluates the re-indexing ops with eval_reindex below, so an
expected value never comes from the product."""
import numpy as np

from band_amd.tflite_synth import FGraph, QGraph

# builtin codes (schema.fbs BuiltinOperator)
DEPTH_TO_SPACE, SPACE_TO_DEPTH, TRANSPOSE, STRIDED_SLICE, SPLIT, SLICE, SPLIT_V = 5, 26, 39, 45, 49, 65, 102
REINDEX_OPS = {DEPTH_TO_SPACE, SPACE_TO_DEPTH, TRANSPOSE, STRIDED_SLICE, SPLIT, SLICE, SPLIT_V}
DTYPES = (np.int8, np.uint8, np.int32, np.float32)


# ---- references ----------------------------------------------------------------
def transpose_ref(x, perm):
    return np.transpose(x, perm)


def slice_ref(x, begin, size):
    return x[tuple(slice(b, None if s == -1 else b + s) for b, s in zip(begin, size))]


def strided_slice_index(begin, end, strides, begin_mask=0, end_mask=0, shrink_axis_mask=0):
    return tuple(int(begin[d]) if shrink_axis_mask >> d & 1 else
                 slice(None if begin_mask >> d & 1 else int(begin[d]), None if end_mask >> d & 1 else int(end[d]),
                       int(strides[d])) for d in range(len(begin)))


def strided_slice_ref(x, begin, end, strides, begin_mask=0, end_mask=0, shrink_axis_mask=0):
    return x[strided_slice_index(begin, end, strides, begin_mask, end_mask, shrink_axis_mask)]


def split_ref(x, num_splits, axis):
    return np.split(x, num_splits, axis)


def split_v_ref(x, sizes, axis):
    sizes = list(sizes)
    if -1 in sizes:
        sizes[sizes.index(-1)] = x.shape[axis] - (sum(sizes) + 1)
    assert sum(sizes) == x.shape[axis]
    return np.split(x, np.cumsum(sizes)[:-1], axis)


def depth_to_space_view(x, bs):
    """(n, h, by, w, bx, c) view: out[n, h bs + by, w bs + bx, c] = in[n, h, w, (by bs + bx) C' + c]"""
    n, h, w, c = x.shape
    return x.reshape(n, h, w, bs, bs, c // (bs * bs)).transpose(0, 1, 3, 2, 4, 5)


def depth_to_space_ref(x, bs):
    n, h, w, c = x.shape
    return depth_to_space_view(x, bs).reshape(n, h * bs, w * bs, c // (bs * bs))


def space_to_depth_view(x, bs):
    """(n, h, w, by, bx, c) view: out[n, h, w, (by bs + bx) C + c] = in[n, h bs + by, w bs + bx, c]"""
    n, h, w, c = x.shape
    return x.reshape(n, h // bs, bs, w // bs, bs, c).transpose(0, 1, 3, 2, 4, 5)


def space_to_depth_ref(x, bs):
    n, h, w, c = x.shape
    return space_to_depth_view(x, bs).reshape(n, h // bs, w // bs, c * bs * bs)


def fill(shape, dtype):
    """arange for 4-byte types, (7 i + 3) mod 251 for 1-byte types: neighbouring elements differ"""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.int64)
    if np.dtype(dtype).itemsize == 4:
        return i.astype(dtype).reshape(shape)
    return ((7 * i + 3) % 251).astype(np.uint8).view(dtype).reshape(shape)


# ---- launcher cases ------------------------------------------------------------
def map_of(x, v):
    """(out_dims, in_stride, in_offset) in elements of the view v of the contiguous array x"""
    assert x.flags.c_contiguous and v.ndim <= 6
    it = x.dtype.itemsize
    off = v.__array_interface__["data"][0] - x.__array_interface__["data"][0]
    assert off % it == 0 and all(s % it == 0 for s in v.strides)
    return list(v.shape), [s // it for s in v.strides], off // it


ROWS, TILE, GATHER = "reindex_rows_kernel", "reindex_tile_kernel", "reindex_gather_kernel"


def launcher_cases():
    """[(id, dtypes, shape, view(x) -> v, kernel or None, misalign)]: the
    expected output is np.ascontiguousarray(v); kernel is the path the case
    pins; misalign uploads the input that many bytes off its buffer's start"""
    one, both = (np.uint8,), (np.uint8, np.float32)
    cases = []

    def add(name, dtypes, shape, view, kernel=None, misalign=0):
        cases.append((name, dtypes, tuple(shape), view, kernel, misalign))

    # rows: run lengths in bytes (a 1-byte run is a single element: a longer tensor of unit rows has no unit stride)
    add("rows_run1", one, (6, 17), lambda x: x[2:3, 5:6], ROWS)
    add("unit_rows", one, (6, 17), lambda x: x[:, 5:6])
    for run in (3, 4, 12, 15, 16, 17, 80):
        add("rows_run%d" % run, one, (6, run + 16), lambda x, r=run: x[:, :r], ROWS)
    # an in_offset that leaves 16 / 8 / 4 / 1 bytes per lane; the last also off a misaligned base pointer
    for off in (16, 8, 4, 1):
        add("rows_offset%d" % off, one, (5, 64), lambda x, o=off: x[:, o:o + 32], ROWS)
    add("rows_offset1_misaligned", one, (5, 64), lambda x: x[:, 1:33], ROWS, 1)
    add("rows_float_offset", (np.float32, np.int32), (5, 24), lambda x: x[:, 3:11], ROWS)
    for k in range(3):
        add("split48_%d" % k, both, (1, 7, 7, 48), lambda x, k=k: x[..., 16 * k:16 * k + 16], ROWS)
    for k in range(2):
        add("split24_%d" % k, both, (1, 7, 7, 24), lambda x, k=k: x[..., 12 * k:12 * k + 12], ROWS)
    add("split5_0", both, (1, 7, 7, 5), lambda x: x[..., :2], ROWS)
    add("split5_1", both, (1, 7, 7, 5), lambda x: x[..., 2:], ROWS)
    add("split_h", both, (2, 6, 5, 8), lambda x: x[:, 2:4], ROWS)
    add("rows_outer1", both, (3, 64), lambda x: x[1:2, 16:48], ROWS)
    # 1.2 M one-byte units: 4,688 workgroups, more than 256 CUs hold at once
    add("rows_many", one, (300000, 8), lambda x: x[:, 2:6], ROWS)
    add("transpose_keeps_channels", both, (2, 5, 7, 8), lambda x: x.transpose(0, 2, 1, 3), ROWS)
    # tile: a transpose whose two tiled extents (the input-contiguous dim and the output's last) are both >= 64;
    # one with a shorter edge is routed to the gather (measured faster there)
    def transposed(dj, dl):
        return TILE if dj >= 64 and dl >= 64 else GATHER
    for shape in ((1, 5, 7, 3), (2, 33, 65, 4), (1, 64, 64, 16), (2, 9, 8, 64)):
        n, h, w, c = shape
        add("nhwc_to_nchw_%dx%dx%dx%d" % shape, both, shape, lambda x: x.transpose(0, 3, 1, 2), transposed(c, h * w))
        add("nchw_to_nhwc_%dx%dx%dx%d" % shape, both, (n, c, h, w), lambda x: x.transpose(0, 2, 3, 1),
            transposed(h * w, c))
    for dj in (63, 64, 65):
        for dl in (63, 64, 65):
            add("tile_edge_%dx%d" % (dj, dl), both, (dl, dj), lambda x: x.T, transposed(dj, dl))
    add("tile_partial_both", both, (130, 67), lambda x: x.T, TILE)
    add("tile_outer_edge", both, (3, 65, 70), lambda x: x.transpose(0, 2, 1), TILE)
    add("tile_two_outer", both, (2, 64, 3, 66), lambda x: x.transpose(2, 0, 3, 1), TILE)
    add("reversal", both, (3, 4, 5, 6), lambda x: x.transpose(3, 2, 1, 0), GATHER)
    add("shuffle5d", both, (1, 14, 14, 2, 16), lambda x: x.transpose(0, 1, 2, 4, 3), GATHER)
    # gather
    add("gather_reverse", both, (5, 37), lambda x: x[:, ::-1], GATHER)
    add("gather_step2", both, (5, 37), lambda x: x[:, ::2], GATHER)
    add("gather_straddle3", one, (7, 6), lambda x: x[:, ::2], GATHER)
    add("gather_all_negative", both, (2, 9, 11, 6), lambda x: x[:, 7:1:-2, 1:10:3, ::-1], GATHER)
    add("gather_partial_group", one, (3, 7), lambda x: x[::-1, ::-1], GATHER)  # 21 bytes: five dwords and one byte
    # depth / space
    for bs in (2, 3):
        for c in (1, 16):
            add("d2s_bs%d_c%d" % (bs, c), both, (2, 3, 5, bs * bs * c), lambda x, b=bs: depth_to_space_view(x, b), ROWS)
            add("s2d_bs%d_c%d" % (bs, c), both, (2, 3 * bs, 5 * bs, c), lambda x, b=bs: space_to_depth_view(x, b), ROWS)
    # the identity and a scalar
    add("identity", both, (2, 3, 4), lambda x: x, ROWS)
    add("scalar", both, (2, 3, 4), lambda x: x[1, 2, 3, ...], ROWS)  # rank 0
    return cases


def reindex_params(x, v, in_ptr, out_ptr):
    from band_amd import _abi
    dims, strides, off = map_of(x, v)
    p = _abi.ReindexParams(elem_bytes=x.dtype.itemsize, rank=len(dims), in_offset=off, input=in_ptr, output=out_ptr)
    for d, (n, s) in enumerate(zip(dims, strides)):
        p.out_dims[d] = n
        p.in_stride[d] = s
    return p


# ---- models --------------------------------------------------------------------
def shuffle_unit(dtype=np.int8):
    """ShuffleNet-style unit at 14x14x32: SPLIT, conv / dw / conv on one half,
    CONCAT, channel shuffle as RESHAPE - TRANSPOSE - RESHAPE, conv"""
    g = QGraph(dtype, seed=41, name="shuffle_unit")
    x = g.input([1, 14, 14, 32], scale=0.05)
    a, b = g.split(x, 2, axis=3)
    b = g.conv(b, 16, k=1)
    b = g.dwconv(b, k=3, act="NONE")
    b = g.conv(b, 16, k=1)
    y = g.concat([a, b], axis=3)
    y = g.reshape(y, [1, 14, 14, 2, 16])
    y = g.transpose(y, (0, 1, 2, 4, 3))
    y = g.reshape(y, [1, 14, 14, 32])
    g.output(g.conv(y, 32, k=1))
    return g.build()


def detector_head(dtype=np.int8):
    """conv, RESHAPE [1,7,7,3,9], TRANSPOSE (0,3,1,2,4), three STRIDED_SLICEs
    (box / objectness / class channels), LOGISTIC on two of them"""
    g = QGraph(dtype, seed=43, name="detector_head")
    x = g.input([1, 7, 7, 8], scale=0.05)
    y = g.conv(x, 27, k=1, act="NONE")
    y = g.reshape(y, [1, 7, 7, 3, 9])
    y = g.transpose(y, (0, 3, 1, 2, 4))
    box = g.strided_slice(y, [0, 0, 0, 0, 0], [1, 3, 7, 7, 4], [1, 1, 1, 1, 1])
    obj = g.strided_slice(y, [0, 0, 0, 0, 4], [1, 3, 7, 7, 5], [1, 1, 1, 1, 1])
    cls = g.strided_slice(y, [0, 0, 0, 0, -4], [0, 0, 0, 0, 0], [1, 1, 1, 1, 1], begin_mask=15, end_mask=31)
    for t in (box, g.logistic(obj), g.logistic(cls)):
        g.output(t)
    return g.build()


def subpixel(dtype=np.int8):
    """SPACE_TO_DEPTH stem at 16x16x3, convs, DEPTH_TO_SPACE tail"""
    g = QGraph(dtype, seed=47, name="subpixel")
    x = g.input([1, 16, 16, 3], scale=0.05)
    y = g.space_to_depth(x, 2)
    y = g.conv(y, 16, k=3)
    y = g.conv(y, 16, k=3)
    y = g.conv(y, 12, k=1, act="NONE")
    g.output(g.depth_to_space(y, 2))
    return g.build()


def float_slice_transpose():
    """a float32 graph (fp16 constants behind DEQUANTIZE): conv, SLICE, TRANSPOSE, SPLIT_V"""
    g = FGraph(seed=53, name="float_slice_transpose")
    x = g.input([1, 8, 8, 4])
    y = g.conv(x, 8, k=3)
    y = g.slice(y, [0, 1, 2, 0], [1, 6, 5, -1])
    y = g.transpose(y, (0, 3, 1, 2))
    a, b = g.split_v(y, [3, -1], axis=1)
    g.output(a)
    g.output(g.relu(b, "RELU6"))
    return g.build()


def batch_axis_transpose():
    """a TRANSPOSE that moves the batch axis: runs, but cannot be job-batched"""
    g = QGraph(np.int8, seed=59, name="batch_axis_transpose")
    x = g.input([1, 4, 4, 8], scale=0.05)
    y = g.conv(x, 8, k=1)
    g.output(g.transpose(y, (1, 0, 2, 3)))
    return g.build()


ZOO = {"shuffle_unit": lambda: shuffle_unit(np.int8), "detector_head_i8": lambda: detector_head(np.int8),
       "detector_head_u8": lambda: detector_head(np.uint8), "subpixel": lambda: subpixel(np.int8),
       "float_slice_transpose": float_slice_transpose}


def zoo_input(buf, seed=0):
    """one random input of the model's (single) input tensor"""
    from oracle.tflite_fb import Model as OModel
    t = OModel(buf).tensors[OModel(buf).inputs[0]]
    rng = np.random.default_rng(seed)
    if t.np_dtype == np.float32:
        return rng.uniform(-1, 1, t.shape).astype(np.float32)
    info = np.iinfo(t.np_dtype)
    return rng.integers(info.min, info.max + 1, t.shape).astype(t.np_dtype)


# ---- the reference of one operator (tests.graph_reference) -------------------------
def eval_reindex(om, o, vals):
    """outputs of re-indexing operator o on vals: the synthesiser's shapes are numpy's"""
    T = om.tensors

    def const(i):
        return [int(v) for v in np.asarray(T[o.inputs[i]].data).reshape(-1)]

    def opt(slot):
        return o.options.scalar(slot, "i", 0) if o.options is not None else 0
    b = o.builtin
    if b == TRANSPOSE:
        return [transpose_ref(vals[o.inputs[0]], const(1))]
    if b == SLICE:
        return [slice_ref(vals[o.inputs[0]], const(1), const(2))]
    if b == STRIDED_SLICE:
        assert opt(2) == 0 and opt(3) == 0
        return [strided_slice_ref(vals[o.inputs[0]], const(1), const(2), const(3), opt(0), opt(1), opt(4))]
    if b == SPLIT:
        return split_ref(vals[o.inputs[1]], len(o.outputs), const(0)[0])
    if b == SPLIT_V:
        return split_v_ref(vals[o.inputs[0]], const(1), const(2)[0])
    if b == DEPTH_TO_SPACE:
        return [depth_to_space_ref(vals[o.inputs[0]], opt(0))]
    assert b == SPACE_TO_DEPTH
    return [space_to_depth_ref(vals[o.inputs[0]], opt(0))]
