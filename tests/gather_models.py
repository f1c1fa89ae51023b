"""Fixtures of GATHER, PACK, UNPACK and TILE: the numpy references, the
launcher case table of bh_gather / CpuGather, the models and the evaluator that
tests.graph_reference.run_reference takes as a further table entry
(run_reference(buf, inputs, table=TABLE + [ENTRY])).

The reference is numpy and nothing else - np.take, np.stack, np.moveaxis,
np.tile - so parity is exact.  One rule is this backend's own:
a runtime GATHER index outside [0, axis_size) reads nothing and its output
slice is zero bytes; gather_ref restates it around np.take."""
import ctypes

import numpy as np

from band_amd.tflite_synth import OPT, FGraph, ModelBuilder, QGraph, Table, text_encoder

GATHER, TILE, PACK, UNPACK = 36, 69, 83, 88
OPS = {GATHER, TILE, PACK, UNPACK}
KERNEL = "gather_rows_kernel"


# ---- references ------------------------------------------------------------------
def gather_ref(params, indices, axis=0):
    """np.take(params, indices, axis); the slice of an index outside [0, axis_size) is zeros"""
    idx = np.asarray(indices, np.int64)
    n = params.shape[axis]
    ok = (idx >= 0) & (idx < n)
    out = np.take(params, np.where(ok, idx, 0), axis)
    if not ok.all():
        out = np.moveaxis(out.reshape(params.shape[:axis] + (idx.size,) + params.shape[axis + 1:]).copy(), axis, 0)
        out[~ok.reshape(-1)] = 0
        out = np.moveaxis(out, 0, axis).reshape(params.shape[:axis] + idx.shape + params.shape[axis + 1:])
    return out


def unpack_ref(x, axis):
    m = np.moveaxis(x, axis, 0)
    return [m[k] for k in range(x.shape[axis])]


def claims(om, o):
    return o.builtin in OPS


def evaluate(om, o, vals):
    """outputs of GATHER / TILE / PACK / UNPACK operator o on vals"""
    def opt(slot):
        return o.options.scalar(slot, "i", 0) if o.options is not None else 0
    b = o.builtin
    if b == GATHER:
        assert opt(1) == 0
        return [gather_ref(vals[o.inputs[0]], vals[o.inputs[1]], opt(0))]
    if b == TILE:
        return [np.tile(vals[o.inputs[0]], [int(v) for v in np.asarray(vals[o.inputs[1]]).reshape(-1)])]
    if b == PACK:
        return [np.stack([vals[t] for t in o.inputs], opt(1))]
    assert b == UNPACK
    return unpack_ref(vals[o.inputs[0]], opt(1))


ENTRY = (claims, evaluate)

# The float32 ops of an encoder block that the oracle does not restate - MEAN
# over the last axis, SQUARED_DIFFERENCE, RSQRT, GELU - go to
# tests.float_harness.op_reference (float64, rounded to float32), and a
# dynamic-range FULLY_CONNECTED to its rule (tests.hybrid_models).
FLOAT_ENCODER_OPS = {40, 99, 76, 150}


def claims_float(om, o):
    return o.builtin in FLOAT_ENCODER_OPS and om.tensors[o.inputs[0]].np_dtype == np.float32


def evaluate_float(om, o, vals):
    from tests import float_harness as H
    ref, _ = H.op_reference(om, o, vals)
    return [np.asarray(ref, np.float32).reshape(om.tensors[o.outputs[0]].shape)]


def claims_hybrid(om, o):
    from tests import hybrid_models as Y
    return Y.is_hybrid_fc(om, o) and om.tensors[o.inputs[0]].np_dtype == np.float32


def evaluate_hybrid(om, o, vals):
    from tests import hybrid_models as Y
    return [np.asarray(Y.hybrid_fc_reference(om, o, vals[o.inputs[0]])).reshape(om.tensors[o.outputs[0]].shape)]


ENTRIES = [ENTRY, (claims_float, evaluate_float), (claims_hybrid, evaluate_hybrid)]


def fill(shape, dtype):
    """no zero and no 0xab byte, neighbouring elements differ: a zero slice, a guard row and a wrong row all show"""
    n = int(np.prod(shape))
    i = np.arange(n, dtype=np.int64)
    if np.dtype(dtype).itemsize == 4:
        return (i + 1).astype(dtype).reshape(shape)
    return ((7 * i + 3) % 170 + 1).astype(np.uint8).view(dtype).reshape(shape)


# ---- launcher cases ----------------------------------------------------------------
GUARD_ROWS = 2
GUARD_BYTE = 0xab


class Case:
    """params of `shape` gathered along `axis` by `indices` (a flat list);
    the table sits `misalign` bytes past a 16-byte boundary; int64_only: the
    values do not fit int32"""

    def __init__(self, name, dtype, shape, axis, indices, misalign=0, int64_only=False):
        self.name, self.dtype, self.shape, self.axis = name, np.dtype(dtype), tuple(shape), axis
        self.indices, self.misalign, self.int64_only = [int(v) for v in indices], misalign, int64_only

    def params(self):
        return fill(self.shape, self.dtype)

    def ref(self):
        return np.ascontiguousarray(gather_ref(self.params(), self.indices, self.axis))

    def counts(self):
        outer = int(np.prod(self.shape[:self.axis], dtype=np.int64))
        inner = int(np.prod(self.shape[self.axis + 1:], dtype=np.int64))
        return outer, self.shape[self.axis], inner

    def guarded_table(self):
        """(bytes, offset of the table): GUARD_ROWS rows (at least 16 bytes) of 0xab on either side, the table
        `misalign` bytes past a multiple of 16"""
        outer, axis_size, inner = self.counts()
        row = inner * self.dtype.itemsize
        front = -(-max(GUARD_ROWS * row, 16) // 16) * 16 + self.misalign
        body = self.params().reshape(-1).view(np.uint8)
        raw = np.full(front + body.size + max(GUARD_ROWS * row, 16) + 16, GUARD_BYTE, np.uint8)
        raw[front:front + body.size] = body
        return raw, front


def launcher_cases():
    cases = []
    mixed = [0, 8, 3, 3, 5, 8, 0, 1]  # index 0, axis_size - 1, repeats
    for b in (1, 3, 4, 8, 12, 16, 20, 48):  # every V of a 1-byte table
        cases.append(Case("u8_row%d" % b, np.uint8, (9, b), 0, mixed))
    cases.append(Case("u8_row1040", np.uint8, (9, 1040), 0, [8, 0, 4, 4, 7]))  # a row longer than a wave's 1 KiB
    for b in (4, 8, 16, 36):
        cases.append(Case("f32_row%d" % b, np.float32, (9, b // 4), 0, mixed))
    cases.append(Case("i32_row16", np.int32, (9, 4), 0, mixed))
    cases.append(Case("i8_row16", np.int8, (9, 16), 0, mixed))
    cases.append(Case("u8_row16_base_off_by_4", np.uint8, (9, 16), 0, mixed, misalign=4))  # V falls back to 4
    cases.append(Case("f32_row16_base_off_by_4", np.float32, (9, 4), 0, mixed, misalign=4))
    cases.append(Case("u8_row16_base_off_by_1", np.uint8, (9, 16), 0, mixed, misalign=1))  # ... to 1
    for dt in (np.uint8, np.float32):
        tag = np.dtype(dt).name
        cases.append(Case("outer3_axis1_%s" % tag, dt, (3, 7, 5), 1, [6, 0, 3, 3]))
        cases.append(Case("outer1_axis1_%s" % tag, dt, (1, 7, 5), 1, [6, 0, 3, 3]))
        cases.append(Case("outer6_last_axis_%s" % tag, dt, (2, 3, 7), 2, [6, 0, 3]))  # inner 1
    for n in (1, 63, 65, 130):
        cases.append(Case("n_idx%d" % n, np.uint8, (11, 48), 0, (np.arange(n) * 7 + 10) % 11))
    cases.append(Case("axis_size1", np.uint8, (1, 12), 0, [0, 0, 0]))
    # out of range, each such that an unguarded address would still fall inside the guard rows
    cases.append(Case("out_of_range_u8", np.uint8, (9, 16), 0, [-1, 0, 9, 8, -2, 10, 4]))
    cases.append(Case("out_of_range_f32_axis1", np.float32, (3, 7, 5), 1, [-1, 6, 7, -2, 8, 0]))
    # a kernel that narrowed these to 32 bits first would read rows 1 and 2
    cases.append(Case("out_of_range_int64", np.uint8, (9, 16), 0, [2**32 + 1, 1, -2**32 + 2, 2], int64_only=True))
    return cases


def gather_params(case, index_dtype, params_ptr, indices_ptr, out_ptr):
    from band_amd import _abi
    outer, axis_size, inner = case.counts()
    return _abi.GatherParams(elem_bytes=case.dtype.itemsize, index_bytes=np.dtype(index_dtype).itemsize, outer=outer,
                             axis_size=axis_size, n_idx=len(case.indices), inner=inner, params=params_ptr,
                             indices=indices_ptr, output=out_ptr)


def run_cpu_gather(lib, case, index_dtype, indices=None):
    """bhx_cpu_gather on the case (or on other `indices`): the output [outer][n_idx][inner]"""
    raw, at = case.guarded_table()
    idx = np.asarray(case.indices if indices is None else indices, index_dtype)
    outer, axis_size, inner = case.counts()
    nbytes = outer * idx.size * inner * case.dtype.itemsize
    out = np.full(nbytes + 32, 0xff, np.uint8)
    table = raw[at:]
    p = gather_params(case, index_dtype, table.ctypes.data, idx.ctypes.data, out.ctypes.data)
    p.n_idx = idx.size
    assert lib.bhx_cpu_gather(ctypes.byref(p)) == 0, lib.bhx_last_error()
    assert (out[nbytes:] == 0xff).all(), "bytes past the output were written"
    return out[:nbytes].view(case.dtype).reshape((outer, idx.size, inner))


# ---- models --------------------------------------------------------------------------
SMALL = dict(tokens=17, dim=48, heads=3, hidden=96, blocks=1, vocab=101)
TEXT_ENCODERS = {
    "text_encoder_i8": lambda **kw: text_encoder(np.int8, **dict(SMALL, **kw)),
    "text_encoder_f32": lambda **kw: text_encoder(np.float32, **dict(SMALL, **kw)),
    "text_encoder_hybrid": lambda **kw: text_encoder(np.float32, hybrid="symmetric", **dict(SMALL, **kw)),
}


def token_ids(buf, seed=0):
    """{input tensor: ids} below the vocabulary size, every position drawn on its own"""
    from oracle.tflite_fb import Model as OModel
    om = OModel(buf)
    t = om.tensors[om.inputs[0]]
    gather = next(o for o in om.operators if o.builtin == GATHER)
    vocab = om.tensors[gather.inputs[0]].shape[0]
    return np.random.default_rng(seed).integers(0, vocab, t.shape).astype(t.np_dtype)


def pack_unpack_tile(dtype=np.int8):
    """UNPACK [1, 3, 5, 8] on axis 1, conv-free: two of the three slices re-packed on axis 2 with the third,
    a [1, 1, 8] slice of the input tiled by [1, 5, 2], and a GATHER of the packed tensor by constant indices"""
    g = QGraph(dtype, seed=71, name="pack_unpack_tile") if np.dtype(dtype).itemsize == 1 else \
        FGraph(seed=71, name="pack_unpack_tile_f32")
    x = g.input([1, 3, 5, 8], scale=0.05)
    a, b, c = g.unpack(x, axis=1)                      # three [1, 5, 8]
    p = g.pack([c, a, b], axis=2)                      # [1, 5, 3, 8]
    row = g.strided_slice(a, [0, 2, 0], [1, 3, 8], [1, 1, 1])  # [1, 1, 8]
    t = g.tile(row, [1, 5, 2])                         # [1, 5, 16]
    q = g.gather(p, [2, 0, 0, 1], axis=2)              # [1, 5, 4, 8]
    for y in (p, t, q):
        g.output(y)
    return g.build()


ZOO = {"pack_unpack_tile_i8": lambda: pack_unpack_tile(np.int8), "pack_unpack_tile_u8": lambda: pack_unpack_tile(np.uint8),
       "pack_unpack_tile_f32": lambda: pack_unpack_tile(np.float32)}


def zoo_input(buf, seed=0):
    from oracle.tflite_fb import Model as OModel
    t = OModel(buf).tensors[OModel(buf).inputs[0]]
    rng = np.random.default_rng(seed)
    if t.np_dtype == np.float32:
        return rng.uniform(-1, 1, t.shape).astype(np.float32)
    info = np.iinfo(t.np_dtype)
    return rng.integers(info.min, info.max + 1, t.shape).astype(t.np_dtype)


def _q(dtype, scale=0.5, zp=3):
    return dict(scale=[scale], zero_point=[zp]) if np.dtype(dtype).itemsize == 1 else {}


def raw_gather(params_shape, indices, axis=0, batch_dims=0, dtype=np.int8, out_scale=0.5, const_params=False,
               runtime_indices=False, index_dtype=np.int32, out_shape=None):
    """one GATHER: params an input (or a constant), indices a constant (or an input)"""
    mb = ModelBuilder("raw_gather")
    idx = np.asarray(indices, index_dtype)
    if const_params:
        x = mb.tensor("params", list(params_shape), dtype, data=fill(params_shape, dtype), **_q(dtype))
    else:
        x = mb.tensor("params", list(params_shape), dtype, **_q(dtype))
        mb.inputs.append(x)
    if runtime_indices:
        it = mb.tensor("indices", list(idx.shape), index_dtype)
        mb.inputs.append(it)
    else:
        it = mb.tensor("indices", list(idx.shape), index_dtype, data=idx)
    ax = axis + len(params_shape) if axis < 0 else axis
    shape = list(params_shape[:ax]) + list(idx.shape) + list(params_shape[ax + 1:]) if out_shape is None else out_shape
    y = mb.tensor("y", shape, dtype, **_q(dtype, out_scale))
    mb.op("GATHER", [x, it], [y], OPT["GatherOptions"], Table().set(0, "i", axis).set(1, "i", batch_dims))
    mb.outputs.append(y)
    return mb.build()


def raw_pack(n, shape=(1, 4, 8), axis=1, dtype=np.int8, odd_scale_at=None):
    mb = ModelBuilder("raw_pack")
    xs = []
    for k in range(n):
        xs.append(mb.tensor("x%d" % k, list(shape), dtype, **_q(dtype, 0.25 if k == odd_scale_at else 0.5)))
        mb.inputs.append(xs[-1])
    out = list(shape[:axis]) + [n] + list(shape[axis:])
    y = mb.tensor("y", out, dtype, **_q(dtype))
    mb.op("PACK", xs, [y], OPT["PackOptions"], Table().set(0, "i", n).set(1, "i", axis))
    mb.outputs.append(y)
    return mb.build()


def raw_unpack(shape=(1, 3, 4, 8), axis=1, dtype=np.int8):
    mb = ModelBuilder("raw_unpack")
    x = mb.tensor("x", list(shape), dtype, **_q(dtype))
    mb.inputs.append(x)
    out = list(shape[:axis]) + list(shape[axis + 1:])
    ys = [mb.tensor("y%d" % k, out, dtype, **_q(dtype)) for k in range(shape[axis])]
    mb.op("UNPACK", [x], ys, OPT["UnpackOptions"], Table().set(0, "i", shape[axis]).set(1, "i", axis))
    mb.outputs += ys
    return mb.build()


def raw_tile(shape, multiples, dtype=np.int8, mult_dtype=np.int32):
    mb = ModelBuilder("raw_tile")
    x = mb.tensor("x", list(shape), dtype, **_q(dtype))
    mb.inputs.append(x)
    mt = mb.tensor("multiples", [len(multiples)], mult_dtype, data=np.asarray(multiples, mult_dtype))
    y = mb.tensor("y", [n * m for n, m in zip(shape, multiples)], dtype, **_q(dtype))
    mb.op("TILE", [x, mt], [y], OPT["TileOptions"], Table())
    mb.outputs.append(y)
    return mb.build()


# TILE maps by the kernel of reindex.hip they reach: (shape, multiples, kernel)
ROWS, RX_GATHER, RX_TILE = "reindex_rows_kernel", "reindex_gather_kernel", "reindex_tile_kernel"
TILE_MAPS = [
    ("mask_rows", (1, 1, 8), (1, 5, 2), ROWS),            # [5][2][8] strides [0][0][1]: merges to [10][8]
    ("inner_repeat", (2, 3, 4), (1, 2, 3), ROWS),         # [2][2][3][3][4], innermost stride 1
    ("class_token", (1, 1, 48), (1, 17, 1), ROWS),
    ("column_broadcast", (1, 6, 1), (1, 1, 16), RX_GATHER),  # innermost stride 0
    ("scalar_fill", (1, 1), (3, 5), RX_GATHER),
    ("column_broadcast_wide", (1, 70, 1), (1, 1, 65), RX_TILE),  # a dim of stride 1 and a zero-stride last, both >= 64
    ("all_axes", (2, 3, 5), (2, 2, 2), ROWS),             # six map dims
]


def tile_map(shape, multiples, dtype, in_ptr, out_ptr):
    """the map ReindexArgs makes of TILE, restated: [m][d] with strides [0][s]; unit dims and multiples of 1 dropped"""
    from band_amd import _abi
    strides = [int(np.prod(shape[d + 1:], dtype=np.int64)) for d in range(len(shape))]
    dims, st = [], []
    for n, m, s in zip(shape, multiples, strides):
        if m > 1:
            dims.append(m)
            st.append(0)
        if n > 1:
            dims.append(n)
            st.append(s)
    p = _abi.ReindexParams(elem_bytes=np.dtype(dtype).itemsize, rank=len(dims), in_offset=0, input=in_ptr, output=out_ptr)
    for d, (n, s) in enumerate(zip(dims, st)):
        p.out_dims[d], p.in_stride[d] = n, s
    return p


def indexed_map(case, index_dtype, params_ptr, indices_ptr, out_ptr):
    """the case as the executor launches it: a bh_reindex_params map [outer][n_idx][inner] that carries the indices"""
    from band_amd import _abi
    outer, axis_size, inner = case.counts()
    p = _abi.ReindexParams(elem_bytes=case.dtype.itemsize, rank=3, in_offset=0, input=params_ptr, output=out_ptr,
                           indices=indices_ptr, index_bytes=np.dtype(index_dtype).itemsize, index_range=axis_size)
    for d, (n, st) in enumerate(zip((outer, len(case.indices), inner), (axis_size * inner, inner, 1))):
        p.out_dims[d], p.in_stride[d] = n, st
    return p
