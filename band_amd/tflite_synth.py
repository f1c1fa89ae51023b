"""Write TFLite schema-v3 flatbuffers and synthesise the BASELINE models.

Five of the six BASELINE.json models are not in the reference's fixtures
(band/test/data/ holds only mobilenet_v2_1.0_224_quant, retinaface, ICN and
magenta), and there is no network, so bench and tests build
them here as .tflite files with the same operator set a TFLite converter
emits.  Weights are synthetic (seeded) unless converted from a real model.

Nothing here is on the hot path: it produces the *input* of IModel::FromPath
(band/backend/tfl/model.cc:25-39).  The writer is dependency-free (no
flatbuffers package): tables are laid out front-to-back with each child
written after its parent so every uoffset is forward, as the format needs.
"""
import struct

import numpy as np

# schema enums
T_FLOAT32, T_FLOAT16, T_INT32, T_UINT8, T_INT8 = 0, 1, 2, 3, 9
T_INT64 = 4
T_INT16 = 7
NP_TO_SCHEMA = {np.dtype(np.float32): T_FLOAT32, np.dtype(np.float16): T_FLOAT16, np.dtype(np.int32): T_INT32,
                np.dtype(np.uint8): T_UINT8, np.dtype(np.int8): T_INT8, np.dtype(np.int64): T_INT64,
                np.dtype(np.int16): T_INT16}
ACT = {"NONE": 0, "RELU": 1, "RELU_N1_TO_1": 2, "RELU6": 3}
OPC = dict(ADD=0, AVERAGE_POOL_2D=1, CONCATENATION=2, CONV_2D=3, DEPTHWISE_CONV_2D=4,
           FULLY_CONNECTED=9, LOGISTIC=14, MAX_POOL_2D=17, MUL=18, RESHAPE=22,
           RESIZE_BILINEAR=23, SOFTMAX=25, CUSTOM=32, PAD=34, SUB=41, QUANTIZE=114,
           DEQUANTIZE=6, RELU=19, RELU_N1_TO_1=20, RELU6=21, PADV2=60, RESIZE_NEAREST_NEIGHBOR=97,
           TRANSPOSE_CONV=67, ARG_MAX=56, ARG_MIN=79,
           DEPTH_TO_SPACE=5, SPACE_TO_DEPTH=26, TRANSPOSE=39, STRIDED_SLICE=45, SPLIT=49, SLICE=65, SPLIT_V=102,
           BATCH_MATMUL=126,
           MEAN=40, RSQRT=76, SQUARED_DIFFERENCE=99, GELU=150,
           GATHER=36, TILE=69, PACK=83, UNPACK=88,
           # from memory of schema.fbs, like the four above; neither has an options table
           TANH=28, EMBEDDING_LOOKUP=7, CAST=53)
# BuiltinOptions union indices
OPT = dict(Conv2DOptions=1, DepthwiseConv2DOptions=2, Pool2DOptions=5, FullyConnectedOptions=8,
           SoftmaxOptions=9, ConcatenationOptions=10, AddOptions=11, ReshapeOptions=17,
           ResizeBilinearOptions=15, MulOptions=21, PadOptions=22, SubOptions=28,
           DequantizeOptions=38, PadV2Options=43, TransposeConvOptions=49, ResizeNearestNeighborOptions=74,
           QuantizeOptions=89, ArgMaxOptions=40, ArgMinOptions=57,
           SpaceToDepthOptions=19, TransposeOptions=26, StridedSliceOptions=32, SplitOptions=35, SliceOptions=44,
           SplitVOptions=79, DepthToSpaceOptions=94,
           # written from memory of schema.fbs; the C++ reader never keys on the union number
           BatchMatMulOptions=101,
           # ... and so are these three
           ReducerOptions=27, SquaredDifferenceOptions=76, GeluOptions=116,
           # ... and these four
           GatherOptions=23, TileOptions=51, PackOptions=59, UnpackOptions=64,
           # ... and this one (slots 0-1 in_data_type, out_data_type)
           CastOptions=37)


# ---------------------------------------------------------------------------
# FlexBuffers map (the encoding of TFLite custom options)
# ---------------------------------------------------------------------------
FBT_INT, FBT_FLOAT, FBT_MAP, FBT_BOOL = 1, 3, 9, 26


def flexbuffer_map(values):
    """A FlexBuffers map of scalars: sorted keys, 8-byte elements.  Layout:
    key strings, the typed key vector, [keys offset, keys width, size],
    elements, one packed type byte per element, then the root (offset, type,
    width)."""
    buf = bytearray()

    def align(n):
        while len(buf) % n:
            buf.append(0)

    keys = sorted(values)
    key_pos = []
    for k in keys:
        key_pos.append(len(buf))
        buf += k.encode() + b"\0"
    align(8)
    buf += struct.pack("<Q", len(keys))
    keys_start = len(buf)
    for kp in key_pos:
        buf += struct.pack("<Q", len(buf) - kp)
    align(8)
    buf += struct.pack("<Q", len(buf) - keys_start)  # keys vector, relative
    buf += struct.pack("<Q", 8)                      # keys element width
    buf += struct.pack("<Q", len(keys))
    map_start = len(buf)
    types = []
    for k in keys:
        v = values[k]
        if isinstance(v, bool):
            buf += struct.pack("<Q", int(v))
            types.append(FBT_BOOL << 2 | 3)
        elif isinstance(v, (int, np.integer)):
            buf += struct.pack("<q", int(v))
            types.append(FBT_INT << 2 | 3)
        else:
            buf += struct.pack("<d", float(v))
            types.append(FBT_FLOAT << 2 | 3)
    buf += bytes(types)
    align(8)
    buf += struct.pack("<Q", len(buf) - map_start)
    buf += bytes([FBT_MAP << 2 | 3, 8])
    return bytes(buf)


# ---------------------------------------------------------------------------
# minimal flatbuffer serializer
# ---------------------------------------------------------------------------
class Table:
    """fields: {slot: (fmt, value)} for scalars, {slot: ('o', obj)} for children."""

    def __init__(self, **kw):
        self.fields = {}

    def set(self, slot, fmt, value):
        self.fields[slot] = (fmt, value)
        return self


class Vec:
    def __init__(self, fmt, values, align=4):
        self.fmt = fmt
        self.values = values
        self.align = align


class VecT:
    def __init__(self, items):
        self.items = items


class Str:
    def __init__(self, s):
        self.s = s.encode() if isinstance(s, str) else bytes(s)


class _Writer:
    def __init__(self):
        self.buf = bytearray()

    def pad_to(self, n, extra=0):
        while (len(self.buf) + extra) % n:
            self.buf.append(0)

    def write(self, obj):
        if isinstance(obj, Table):
            return self._table(obj)
        if isinstance(obj, Vec):
            return self._vec(obj)
        if isinstance(obj, VecT):
            return self._vect(obj)
        if isinstance(obj, Str):
            self.pad_to(4)
            pos = len(self.buf)
            self.buf += struct.pack("<I", len(obj.s)) + obj.s + b"\0"
            return pos
        raise TypeError(obj)

    def _vec(self, v):
        if isinstance(v.values, (bytes, bytearray, np.ndarray)):
            raw = bytes(np.ascontiguousarray(v.values).tobytes()) if isinstance(v.values, np.ndarray) else bytes(v.values)
            n = len(raw) // struct.calcsize("<" + v.fmt)
        else:
            raw = b"".join(struct.pack("<" + v.fmt, x) for x in v.values)
            n = len(v.values)
        self.pad_to(max(v.align, 4), extra=4)
        pos = len(self.buf)
        self.buf += struct.pack("<I", n) + raw
        return pos

    def _vect(self, v):
        self.pad_to(4)
        pos = len(self.buf)
        self.buf += struct.pack("<I", len(v.items))
        slots = []
        for _ in v.items:
            slots.append(len(self.buf))
            self.buf += b"\0\0\0\0"
        for slot, item in zip(slots, v.items):
            cpos = self.write(item)
            struct.pack_into("<I", self.buf, slot, cpos - slot)
        return pos

    def _table(self, t):
        slots = sorted(t.fields)
        nslots = (max(slots) + 1) if slots else 0
        # field layout inside the table: scalars by size (desc), then offsets
        items = []
        for s in slots:
            fmt, val = t.fields[s]
            size = 4 if fmt == "o" else struct.calcsize("<" + fmt)
            items.append((size, s, fmt, val))
        items.sort(key=lambda x: -x[0])
        layout = {}
        off = 4  # soffset to vtable
        for size, s, fmt, val in items:
            off = (off + size - 1) // size * size
            layout[s] = off
            off += size
        tsize = off
        vt = struct.pack("<HH", 4 + 2 * nslots, tsize) + b"".join(
            struct.pack("<H", layout.get(i, 0)) for i in range(nslots))
        self.pad_to(2)
        vt_pos = len(self.buf)
        self.buf += vt
        self.pad_to(8)
        tpos = len(self.buf)
        self.buf += bytearray(tsize)
        struct.pack_into("<i", self.buf, tpos, tpos - vt_pos)
        children = []
        for size, s, fmt, val in items:
            p = tpos + layout[s]
            if fmt == "o":
                children.append((p, val))
            else:
                struct.pack_into("<" + fmt, self.buf, p, val)
        for p, child in children:
            cpos = self.write(child)
            struct.pack_into("<I", self.buf, p, cpos - p)
        return tpos


def serialize(root):
    w = _Writer()
    w.buf += b"\0\0\0\0TFL3"
    rpos = w.write(root)
    struct.pack_into("<I", w.buf, 0, rpos)
    return bytes(w.buf)


# ---------------------------------------------------------------------------
# model description -> flatbuffer
# ---------------------------------------------------------------------------
class ModelBuilder:
    """Collects tensors / buffers / operators of one subgraph."""

    def __init__(self, description="band_amd synthetic"):
        self.tensors = []   # dicts
        self.buffers = [b""]  # buffer 0 is the empty sentinel
        self.ops = []
        self.opcodes = []   # (builtin, custom)
        self.inputs = []
        self.outputs = []
        self.description = description

    def tensor(self, name, shape, dtype, scale=None, zero_point=None, qdim=0, data=None):
        buf = 0
        if data is not None:
            arr = np.ascontiguousarray(np.asarray(data, dtype=dtype).reshape(shape))
            self.buffers.append(arr.tobytes())
            buf = len(self.buffers) - 1
        self.tensors.append(dict(name=name, shape=list(shape), type=NP_TO_SCHEMA[np.dtype(dtype)],
                                 buffer=buf, scale=scale, zero_point=zero_point, qdim=qdim))
        return len(self.tensors) - 1

    def op(self, builtin, inputs, outputs, options_type=0, options=None, custom=None, custom_options=None):
        key = (OPC[builtin] if isinstance(builtin, str) else builtin, custom)
        if key not in self.opcodes:
            self.opcodes.append(key)
        self.ops.append(dict(opcode=self.opcodes.index(key), inputs=list(inputs), outputs=list(outputs),
                             options_type=options_type, options=options, custom_options=custom_options))
        return len(self.ops) - 1

    def build(self):
        tens = []
        for t in self.tensors:
            tt = Table().set(0, "o", Vec("i", t["shape"])).set(1, "b", t["type"]).set(2, "I", t["buffer"])
            tt.set(3, "o", Str(t["name"]))
            if t["scale"] is not None:
                sc = [float(x) for x in np.atleast_1d(t["scale"])]
                zp = [int(x) for x in np.atleast_1d(t["zero_point"] if t["zero_point"] is not None else 0)]
                if len(zp) != len(sc):
                    zp = zp * len(sc) if len(zp) == 1 else zp
                q = Table().set(2, "o", Vec("f", sc)).set(3, "o", Vec("q", zp)).set(6, "i", int(t["qdim"]))
                tt.set(4, "o", q)
            tens.append(tt)
        ops = []
        for o in self.ops:
            ot = Table().set(0, "I", o["opcode"]).set(1, "o", Vec("i", o["inputs"])).set(2, "o", Vec("i", o["outputs"]))
            if o["options_type"]:
                ot.set(3, "B", o["options_type"]).set(4, "o", o["options"])
            if o.get("custom_options") is not None:
                ot.set(5, "o", Vec("B", o["custom_options"]))  # custom_options_format FLEXBUFFERS (0)
            ops.append(ot)
        sg = (Table().set(0, "o", VecT(tens)).set(1, "o", Vec("i", self.inputs))
              .set(2, "o", Vec("i", self.outputs)).set(3, "o", VecT(ops)).set(4, "o", Str("main")))
        codes = []
        for b, c in self.opcodes:
            oc = Table().set(0, "b", min(b, 127)).set(2, "i", 1).set(3, "i", b)
            if c:
                oc.set(1, "o", Str(c))
            codes.append(oc)
        bufs = [Table() if not b else Table().set(0, "o", Vec("B", b, align=16)) for b in self.buffers]
        root = (Table().set(0, "I", 3).set(1, "o", VecT(codes)).set(2, "o", VecT([sg]))
                .set(3, "o", Str(self.description)).set(4, "o", VecT(bufs)))
        return serialize(root)


def conv_options(padding, stride, act, dilation=1):
    return (Table().set(0, "b", 0 if padding == "SAME" else 1).set(1, "i", stride).set(2, "i", stride)
            .set(3, "b", ACT[act]).set(4, "i", dilation).set(5, "i", dilation))


def dw_options(padding, stride, act, dm=1, dilation=1):
    return (Table().set(0, "b", 0 if padding == "SAME" else 1).set(1, "i", stride).set(2, "i", stride)
            .set(3, "i", dm).set(4, "b", ACT[act]).set(5, "i", dilation).set(6, "i", dilation))


def pool_options(padding, stride, filt, act="NONE"):
    return (Table().set(0, "b", 0 if padding == "SAME" else 1).set(1, "i", stride).set(2, "i", stride)
            .set(3, "i", filt[1]).set(4, "i", filt[0]).set(5, "b", ACT[act]))


def act_options(act="NONE"):
    return Table().set(0, "b", ACT[act])


def bmm_options(adj_x=False, adj_y=False, asymmetric_quantize_inputs=False):
    """BatchMatMulOptions: adj_x, adj_y, asymmetric_quantize_inputs (fields 0-2)"""
    return (Table().set(0, "b", int(adj_x)).set(1, "b", int(adj_y)).set(2, "b", int(asymmetric_quantize_inputs)))


def _bmm_shape(sa, sb, adj_x, adj_y):
    """(output shape, K) of BATCH_MATMUL on shapes sa, sb: numpy matmul after the adjoints"""
    ma = list(sa[-2:])[::-1] if adj_x else list(sa[-2:])
    mb_ = list(sb[-2:])[::-1] if adj_y else list(sb[-2:])
    assert ma[1] == mb_[0], "BATCH_MATMUL: K differs"
    lead = np.broadcast_shapes(tuple(sa[:-2]), tuple(sb[:-2]))
    return [int(v) for v in lead] + [ma[0], mb_[1]], ma[1]


class _ReindexOps:
    """The re-indexing ops of QGraph and FGraph: TRANSPOSE, STRIDED_SLICE,
    SLICE, SPLIT, SPLIT_V, SPACE_TO_DEPTH, DEPTH_TO_SPACE, UNPACK, TILE, and
    GATHER and PACK beside them.  They draw nothing from the RNG; an output
    inherits the input's quantisation (the ops copy bytes).  Index arguments
    are constant int32 tensors, except GATHER's indices, which may be a tensor
    of the graph."""

    def _re_out(self, x, shape):
        shape = [int(v) for v in shape]
        return self._like(x, shape=shape) if hasattr(self, "_like") else self._act(shape)

    def _re_ints(self, kind, values):
        v = np.asarray(values, np.int32)
        return self.mb.tensor(self._name(kind), list(v.shape), np.int32, data=v)

    def transpose(self, x, perm):
        shp = self.meta[x][0]
        pt = self._re_ints("perm", list(perm))
        y = self._re_out(x, [shp[p] for p in perm])
        self.mb.op("TRANSPOSE", [x, pt], [y], OPT["TransposeOptions"], Table())
        return y

    def slice(self, x, begin, size):
        """x[b0:b0+s0, ...]; size -1 = to the end"""
        shp = self.meta[x][0]
        bt, st = self._re_ints("begin", list(begin)), self._re_ints("size", list(size))
        y = self._re_out(x, [shp[d] - begin[d] if size[d] == -1 else size[d] for d in range(len(shp))])
        self.mb.op("SLICE", [x, bt, st], [y], OPT["SliceOptions"], Table())
        return y

    def strided_slice(self, x, begin, end, strides, begin_mask=0, end_mask=0, shrink_axis_mask=0,
                      ellipsis_mask=0, new_axis_mask=0):
        """numpy basic indexing x[b:e:s] per axis; a begin_mask / end_mask bit
        drops that bound, a shrink_axis_mask bit makes the axis the index x[b]"""
        shp = self.meta[x][0]
        idx = tuple(int(begin[d]) if shrink_axis_mask >> d & 1 else
                    slice(None if begin_mask >> d & 1 else int(begin[d]),
                          None if end_mask >> d & 1 else int(end[d]), int(strides[d])) for d in range(len(shp)))
        out_shape = np.broadcast_to(np.int8(0), shp)[idx].shape
        ins = [x, self._re_ints("begin", list(begin)), self._re_ints("end", list(end)),
               self._re_ints("strides", list(strides))]
        y = self._re_out(x, out_shape)
        opt = (Table().set(0, "i", begin_mask).set(1, "i", end_mask).set(2, "i", ellipsis_mask)
               .set(3, "i", new_axis_mask).set(4, "i", shrink_axis_mask))
        self.mb.op("STRIDED_SLICE", ins, [y], OPT["StridedSliceOptions"], opt)
        return y

    def split(self, x, num_splits, axis):
        """np.split(x, num_splits, axis): a list of outputs"""
        shp = list(self.meta[x][0])
        at = self.mb.tensor(self._name("axis"), [], np.int32, data=np.array(axis, np.int32))
        shp[axis] //= num_splits
        ys = [self._re_out(x, shp) for _ in range(num_splits)]
        self.mb.op("SPLIT", [at, x], ys, OPT["SplitOptions"], Table().set(0, "i", num_splits))
        return ys

    def split_v(self, x, sizes, axis):
        """np.split at the running sums of `sizes` (one may be -1: the rest)"""
        shp = list(self.meta[x][0])
        st = self._re_ints("size_splits", list(sizes))
        at = self.mb.tensor(self._name("axis"), [], np.int32, data=np.array(axis, np.int32))
        known = sum(s for s in sizes if s != -1)
        ys = []
        for s in sizes:
            shp[axis] = self.meta[x][0][axis] - known if s == -1 else s
            ys.append(self._re_out(x, shp))
        self.mb.op("SPLIT_V", [x, st, at], ys, OPT["SplitVOptions"], Table().set(0, "i", len(sizes)))
        return ys

    def space_to_depth(self, x, block_size):
        n, h, w, c = self.meta[x][0]
        y = self._re_out(x, [n, h // block_size, w // block_size, c * block_size * block_size])
        self.mb.op("SPACE_TO_DEPTH", [x], [y], OPT["SpaceToDepthOptions"], Table().set(0, "i", block_size))
        return y

    def depth_to_space(self, x, block_size):
        n, h, w, c = self.meta[x][0]
        y = self._re_out(x, [n, h * block_size, w * block_size, c // (block_size * block_size)])
        self.mb.op("DEPTH_TO_SPACE", [x], [y], OPT["DepthToSpaceOptions"], Table().set(0, "i", block_size))
        return y

    def gather(self, params, indices, axis=0, batch_dims=0, index_dtype=np.int32):
        """np.take(params, indices, axis).  `indices` is a tensor of the graph (an
        int32 / int64 input) or a list / array, which becomes a constant of
        index_dtype; the output inherits params' quantisation"""
        shp = self.meta[params][0]
        if isinstance(indices, (list, tuple, np.ndarray)):
            v = np.asarray(indices, index_dtype)
            ishape = list(v.shape)
            indices = self.mb.tensor(self._name("indices"), ishape, index_dtype, data=v)
        else:
            ishape = self.meta[indices][0]
        ax = axis + len(shp) if axis < 0 else axis
        y = self._re_out(params, list(shp[:ax]) + list(ishape) + list(shp[ax + 1:]))
        self.mb.op("GATHER", [params, indices], [y], OPT["GatherOptions"],
                   Table().set(0, "i", axis).set(1, "i", batch_dims))
        return y

    def cast(self, x, dtype):
        """CAST to dtype (uint8, int32, int64 or float32) of a tensor without quantisation; the output has none"""
        shp = list(self.meta[x][0])
        y = self.mb.tensor(self._name("cast"), shp, dtype)
        self.meta[y] = (shp, None, None)
        src = self.mb.tensors[x]["type"]
        self.mb.op("CAST", [x], [y], OPT["CastOptions"], Table().set(0, "b", src).set(1, "b", NP_TO_SCHEMA[np.dtype(dtype)]))
        return y

    def embedding_lookup(self, ids, table):
        """EMBEDDING_LOOKUP: np.take(table, ids, 0) with the operands in TFLite's order (ids first); the output
        inherits the table's quantisation"""
        shp = self.meta[table][0]
        y = self._re_out(table, list(self.meta[ids][0]) + list(shp[1:]))
        self.mb.op("EMBEDDING_LOOKUP", [ids, table], [y])
        return y

    def pack(self, xs, axis=0):
        """np.stack(xs, axis); the inputs share one shape and, 8-bit, one quantisation"""
        shp = list(self.meta[xs[0]][0])
        ax = axis + len(shp) + 1 if axis < 0 else axis
        y = self._re_out(xs[0], shp[:ax] + [len(xs)] + shp[ax:])
        self.mb.op("PACK", list(xs), [y], OPT["PackOptions"], Table().set(0, "i", len(xs)).set(1, "i", axis))
        return y

    def unpack(self, x, axis=0):
        """[np.moveaxis(x, axis, 0)[k] for k in range(x.shape[axis])]: a list of outputs"""
        shp = list(self.meta[x][0])
        ax = axis + len(shp) if axis < 0 else axis
        ys = [self._re_out(x, shp[:ax] + shp[ax + 1:]) for _ in range(shp[ax])]
        self.mb.op("UNPACK", [x], ys, OPT["UnpackOptions"], Table().set(0, "i", shp[ax]).set(1, "i", axis))
        return ys

    def tile(self, x, multiples):
        """np.tile(x, multiples), one multiple per dim"""
        shp = self.meta[x][0]
        mt = self._re_ints("multiples", list(multiples))
        y = self._re_out(x, [n * m for n, m in zip(shp, multiples)])
        self.mb.op("TILE", [x, mt], [y], OPT["TileOptions"], Table())
        return y


# ---------------------------------------------------------------------------
# quantised graph construction with synthetic (seeded) weights
# ---------------------------------------------------------------------------
class QGraph(_ReindexOps):
    """Builds an int8 (per-channel) or uint8 (per-tensor) NHWC graph.

    Scales mimic converter output (RELU6 tensors at 6/255) and filter scales
    are chosen per layer so activations stay spread over the 8-bit range
    instead of collapsing or saturating, which keeps bit-exact checks
    meaningful (BASELINE.md's log-uniform [1e-3, 2e-2] filter scales collapse
    a 65-op network to constants within a few layers).
    """

    def __init__(self, dtype=np.int8, seed=0, name="model"):
        self.dtype = np.dtype(dtype)
        self.rng = np.random.default_rng(seed)
        self.mb = ModelBuilder(name)
        self.n = 0
        self.meta = {}  # tensor -> (shape, scale, zp)
        self.fshape = {}  # float32 tensor -> shape

    def _name(self, kind):
        self.n += 1
        return "%s_%d" % (kind, self.n)

    def _act_zp(self):
        return int(self.rng.integers(-20, 21)) if self.dtype == np.int8 else int(self.rng.integers(108, 149))

    def act_tensor(self, shape, scale, zp, kind="act"):
        t = self.mb.tensor(self._name(kind), shape, self.dtype, scale=[scale], zero_point=[zp])
        self.meta[t] = (list(shape), scale, zp)
        return t

    def input(self, shape, scale=0.0078125, zp=None, dtype=None):
        """a model input; dtype np.int32 / np.int64: an index tensor (token ids) without quantisation"""
        if dtype is not None:
            t = self.mb.tensor(self._name("input"), list(shape), dtype)
            self.meta[t] = (list(shape), None, None)
            self.mb.inputs.append(t)
            return t
        zp = (0 if self.dtype == np.int8 else 128) if zp is None else zp
        t = self.act_tensor(shape, scale, zp, "input")
        self.mb.inputs.append(t)
        return t

    def output(self, t):
        self.mb.outputs.append(t)

    def _out_q(self, act, s_in):
        """Output (scale, zero point) the way converted models look: RELU6/RELU
        outputs cover [0, 6] (scale 6/255, zero point at the range bottom);
        linear outputs keep the input scale around a small zero point."""
        if act in ("RELU6", "RELU"):
            return 6.0 / 255.0, (-128 if self.dtype == np.int8 else 0)
        return float(s_in), self._act_zp()

    def _weights(self, shape, out_c, qdim, s_in, s_out, K):
        # filter scale chosen so sum_k x*w lands ~40 output LSBs wide
        # (|x - zp| ~ 45 LSB, |w| ~ 73 LSB), jittered per channel
        base = 40.0 * s_out / (s_in * np.sqrt(K) * 45.0 * 73.0)
        if self.dtype == np.int8:
            w = self.rng.integers(-127, 128, size=shape).astype(np.int8)
            ws = (base * np.exp(self.rng.uniform(-0.4, 0.4, size=out_c))).astype(np.float32)
            wt = self.mb.tensor(self._name("weights"), shape, np.int8, scale=ws, zero_point=[0] * out_c,
                                qdim=qdim, data=w)
            return wt, ws
        w = self.rng.integers(0, 256, size=shape).astype(np.uint8)
        ws = np.array([base * np.exp(self.rng.uniform(-0.4, 0.4))], np.float32)
        wt = self.mb.tensor(self._name("weights"), shape, np.uint8, scale=ws,
                            zero_point=[int(self.rng.integers(125, 132))], data=w)
        return wt, ws

    def _bias(self, out_c, in_scale, ws, K):
        lim = max(1, int(np.sqrt(K) * 45 * 73 / 3))
        b = self.rng.integers(-lim, lim + 1, size=out_c).astype(np.int32)
        bs = (np.float32(in_scale) * (ws if len(ws) > 1 else np.repeat(ws, out_c))).astype(np.float32)
        return self.mb.tensor(self._name("bias"), [out_c], np.int32, scale=bs, zero_point=[0] * out_c, data=b)

    def conv(self, x, out_c, k=1, stride=1, act="RELU6", padding="SAME", dilation=1, out_scale=None,
             bias_offset_lsb=0, groups=1):
        """CONV_2D; `out_scale` overrides the output scale and
        `bias_offset_lsb` shifts every output channel by that many output
        LSBs (a detection head's class prior); `groups` > 1 writes the grouped
        filter [out_c, k, k, c // groups] (output channel o reads the input
        channels of group o // (out_c // groups) only)"""
        shp, s_in, _ = self.meta[x]
        b, h, w, c = shp
        assert c % groups == 0 and out_c % groups == 0, "groups must divide both channel counts"
        s_out, zp = self._out_q(act, s_in)
        if out_scale is not None:
            s_out = float(out_scale)
        K = k * k * c // groups
        wt, ws = self._weights([out_c, k, k, c // groups], out_c, 0, s_in, s_out, K)
        bt = self._bias(out_c, s_in, ws, K)
        if bias_offset_lsb:
            bias = self.mb.tensors[bt]
            bufi = bias["buffer"]
            vals = np.frombuffer(self.mb.buffers[bufi], np.int32).copy()
            wsc = ws if len(ws) > 1 else np.repeat(ws, out_c)
            vals += np.round(bias_offset_lsb * s_out / (s_in * wsc.astype(np.float64))).astype(np.int32)
            self.mb.buffers[bufi] = vals.tobytes()
        eff = (k - 1) * dilation + 1
        oh = (h + stride - 1) // stride if padding == "SAME" else (h + stride - eff) // stride
        ow = (w + stride - 1) // stride if padding == "SAME" else (w + stride - eff) // stride
        y = self.act_tensor([b, oh, ow, out_c], s_out, zp)
        self.mb.op("CONV_2D", [x, wt, bt], [y], OPT["Conv2DOptions"], conv_options(padding, stride, act, dilation))
        return y

    def dwconv(self, x, k=3, stride=1, act="RELU6", padding="SAME", dm=1, dilation=1):
        shp, s_in, _ = self.meta[x]
        b, h, w, c = shp
        oc = c * dm
        s_out, zp = self._out_q(act, s_in)
        wt, ws = self._weights([1, k, k, oc], oc, 3, s_in, s_out, k * k)
        bt = self._bias(oc, s_in, ws, k * k)
        eff = (k - 1) * dilation + 1
        oh = (h + stride - 1) // stride if padding == "SAME" else (h + stride - eff) // stride
        ow = (w + stride - 1) // stride if padding == "SAME" else (w + stride - eff) // stride
        y = self.act_tensor([b, oh, ow, oc], s_out, zp)
        self.mb.op("DEPTHWISE_CONV_2D", [x, wt, bt], [y], OPT["DepthwiseConv2DOptions"],
                   dw_options(padding, stride, act, dm, dilation))
        return y

    def add(self, a, b, act="NONE"):
        shp, sa, _ = self.meta[a]
        _, sb, _ = self.meta[b]
        y = self.act_tensor(shp, float(max(sa, sb) * 1.4), self._act_zp())
        self.mb.op("ADD", [a, b], [y], OPT["AddOptions"], act_options(act))
        return y

    def avgpool(self, x, filt, stride=1, padding="VALID"):
        shp, s, z = self.meta[x]
        b, h, w, c = shp
        oh = (h + stride - filt[0]) // stride if padding == "VALID" else (h + stride - 1) // stride
        ow = (w + stride - filt[1]) // stride if padding == "VALID" else (w + stride - 1) // stride
        y = self.act_tensor([b, oh, ow, c], s, z)
        self.mb.op("AVERAGE_POOL_2D", [x], [y], OPT["Pool2DOptions"], pool_options(padding, stride, filt))
        return y

    def maxpool(self, x, filt, stride, padding="SAME"):
        shp, s, z = self.meta[x]
        b, h, w, c = shp
        oh = (h + stride - filt[0]) // stride if padding == "VALID" else (h + stride - 1) // stride
        ow = (w + stride - filt[1]) // stride if padding == "VALID" else (w + stride - 1) // stride
        y = self.act_tensor([b, oh, ow, c], s, z)
        self.mb.op("MAX_POOL_2D", [x], [y], OPT["Pool2DOptions"], pool_options(padding, stride, filt))
        return y

    def reshape(self, x, shape):
        _, s, z = self.meta[x]
        st = self.mb.tensor(self._name("shape"), [len(shape)], np.int32, data=np.array(shape, np.int32))
        y = self.act_tensor(list(shape), s, z)
        self.mb.op("RESHAPE", [x, st], [y], OPT["ReshapeOptions"], Table().set(0, "o", Vec("i", list(shape))))
        return y

    def fully_connected(self, x, units, act="NONE", keep_num_dims=False, out_scale=None):
        """FULLY_CONNECTED; keep_num_dims keeps the input's leading dims
        ([1, T, C] -> [1, T, units]) instead of flattening them to rows;
        out_scale overrides the output scale"""
        shp, s_in, _ = self.meta[x]
        depth = shp[-1]
        rows = int(np.prod(shp)) // depth
        w = (self.rng.integers(-127, 128, size=(units, depth)).astype(np.int8) if self.dtype == np.int8
             else self.rng.integers(0, 256, size=(units, depth)).astype(np.uint8))
        ws = np.array([np.exp(self.rng.uniform(np.log(1e-3), np.log(2e-2)))], np.float32)
        wzp = 0 if self.dtype == np.int8 else int(self.rng.integers(125, 132))
        s_out, zp = self._out_q(act, s_in)
        if out_scale is not None:
            s_out = float(out_scale)
        ws = np.array([40.0 * s_out / (s_in * np.sqrt(depth) * 45.0 * 73.0)], np.float32)
        wt = self.mb.tensor(self._name("fc_weights"), [units, depth], self.dtype, scale=ws, zero_point=[wzp], data=w)
        bt = self._bias(units, s_in, ws, depth)
        y = self.act_tensor(list(shp[:-1]) + [units] if keep_num_dims else [rows, units], s_out, zp)
        opt = act_options(act)
        if keep_num_dims:
            opt.set(2, "b", 1)
        self.mb.op("FULLY_CONNECTED", [x, wt, bt], [y], OPT["FullyConnectedOptions"], opt)
        return y

    def batch_matmul(self, a, b, adj_x=False, adj_y=False, out_scale=None, out_zp=None):
        """BATCH_MATMUL of two activations (numpy matmul over the last two
        dims after adj_x / adj_y, leading dims broadcast).  The default output
        scale puts sum_k (a - z_a)(b - z_b) of ~45-LSB operands ~32 output
        LSBs wide."""
        sa, s_a, _ = self.meta[a]
        sb, s_b, _ = self.meta[b]
        shape, K = _bmm_shape(sa, sb, adj_x, adj_y)
        s_out = float(out_scale) if out_scale is not None else float(s_a * s_b * np.sqrt(K) * 45.0 * 45.0 / 32.0)
        y = self.act_tensor(shape, s_out, self._act_zp() if out_zp is None else out_zp)
        self.mb.op("BATCH_MATMUL", [a, b], [y], OPT["BatchMatMulOptions"], bmm_options(adj_x, adj_y))
        return y

    # --- glue ops ------------------------------------------------------------
    def _like(self, x, shape=None, scale=None, zp=None):
        shp, s, z = self.meta[x]
        return self.act_tensor(list(shape if shape is not None else shp), s if scale is None else scale,
                               z if zp is None else zp)

    def quantize(self, x, scale, zp):
        """QUANTIZE (requantize) to new 8-bit params"""
        y = self._like(x, scale=scale, zp=zp)
        self.mb.op("QUANTIZE", [x], [y], OPT["QuantizeOptions"], Table())
        return y

    def concat(self, xs, axis=3):
        """CONCATENATION; int8 inputs are requantized to the first input's
        params first (what the converter does), uint8 ones are rescaled by the
        op itself (ConcatenationWithScaling)"""
        shp0, s0, z0 = self.meta[xs[0]]
        ins = []
        for x in xs:
            _, s, z = self.meta[x]
            if self.dtype == np.int8 and (s != s0 or z != z0):
                x = self.quantize(x, s0, z0)
            ins.append(x)
        shape = list(shp0)
        shape[axis] = sum(self.meta[x][0][axis] for x in ins)
        s_out = s0 if self.dtype == np.int8 else float(max(self.meta[x][1] for x in ins))
        z_out = z0 if self.dtype == np.int8 else self._act_zp()
        y = self.act_tensor(shape, s_out, z_out)
        self.mb.op("CONCATENATION", ins, [y], OPT["ConcatenationOptions"], Table().set(0, "i", axis).set(1, "b", 0))
        return y

    def pad(self, x, pads):
        """PAD with [[before, after]] per dim (quantized pad = output zero point)"""
        shp, _, _ = self.meta[x]
        pt = self.mb.tensor(self._name("paddings"), [len(shp), 2], np.int32, data=np.array(pads, np.int32))
        y = self._like(x, shape=[shp[d] + pads[d][0] + pads[d][1] for d in range(len(shp))])
        self.mb.op("PAD", [x, pt], [y], OPT["PadOptions"], Table())
        return y

    def relu(self, x, kind="RELU"):
        shp, s, z = self.meta[x]
        lo = {"RELU": 0.0, "RELU6": 0.0, "RELU_N1_TO_1": -1.0}[kind]
        hi = {"RELU": None, "RELU6": 6.0, "RELU_N1_TO_1": 1.0}[kind]
        qmin = -128 if self.dtype == np.int8 else 0
        span = (hi if hi is not None else s * 200.0) - lo
        scale = float(span / 255.0)
        y = self.act_tensor(shp, scale, int(qmin - round(lo / scale)))
        self.mb.op(kind, [x], [y])
        return y

    def logistic(self, x):
        zp = -128 if self.dtype == np.int8 else 0
        y = self._like(x, scale=1.0 / 256.0, zp=zp)
        self.mb.op("LOGISTIC", [x], [y])
        return y

    def tanh(self, x):
        """TANH; the output covers [-1, 1): scale 1 / 128 around the middle of the range"""
        y = self._like(x, scale=1.0 / 128.0, zp=0 if self.dtype == np.int8 else 128)
        self.mb.op("TANH", [x], [y])
        return y

    def softmax(self, x, beta=1.0):
        zp = -128 if self.dtype == np.int8 else 0
        y = self._like(x, scale=1.0 / 256.0, zp=zp)
        self.mb.op("SOFTMAX", [x], [y], OPT["SoftmaxOptions"], Table().set(0, "f", float(beta)))
        return y

    def resize(self, x, size, bilinear=False, align_corners=False, half_pixel_centers=False):
        shp, _, _ = self.meta[x]
        st = self.mb.tensor(self._name("size"), [2], np.int32, data=np.array(size, np.int32))
        y = self._like(x, shape=[shp[0], size[0], size[1], shp[3]])
        if bilinear:
            opt = Table().set(2, "b", int(align_corners)).set(3, "b", int(half_pixel_centers))
            self.mb.op("RESIZE_BILINEAR", [x, st], [y], OPT["ResizeBilinearOptions"], opt)
        else:
            opt = Table().set(0, "b", int(align_corners)).set(1, "b", int(half_pixel_centers))
            self.mb.op("RESIZE_NEAREST_NEIGHBOR", [x, st], [y], OPT["ResizeNearestNeighborOptions"], opt)
        return y

    def transpose_conv(self, x, out_c, k=3, stride=2, padding="SAME", bias=True):
        """TRANSPOSE_CONV (int8 per-channel): output = input * stride (SAME)
        or (input - 1) * stride + k (VALID)"""
        shp, s_in, _ = self.meta[x]
        b, h, w, c = shp
        oh = h * stride if padding == "SAME" else (h - 1) * stride + k
        ow = w * stride if padding == "SAME" else (w - 1) * stride + k
        s_out, zp = float(s_in) * 1.5, self._act_zp()
        K = max(1, k * k * c // (stride * stride))
        wt, ws = self._weights([out_c, k, k, c], out_c, 0, s_in, s_out, K)
        shape_t = self.mb.tensor(self._name("out_shape"), [4], np.int32, data=np.array([b, oh, ow, out_c], np.int32))
        ins = [shape_t, wt, x]
        if bias:
            ins.append(self._bias(out_c, s_in, ws, K))
        y = self.act_tensor([b, oh, ow, out_c], s_out, zp)
        opt = Table().set(0, "b", 0 if padding == "SAME" else 1).set(1, "i", stride).set(2, "i", stride)
        self.mb.op("TRANSPOSE_CONV", ins, [y], OPT["TransposeConvOptions"], opt)
        return y

    def dequantize(self, x):
        shp, _, _ = self.meta[x]
        y = self.mb.tensor(self._name("float"), shp, np.float32)
        self.mb.op("DEQUANTIZE", [x], [y], OPT["DequantizeOptions"], Table())
        self.fshape[y] = list(shp)
        return y

    def float_add(self, a, b, act="NONE"):
        """float32 ADD (a CPU-worker op: the GPU set is 8-bit only)"""
        y = self.mb.tensor(self._name("float"), self.fshape[a], np.float32)
        self.mb.op("ADD", [a, b], [y], OPT["AddOptions"], act_options(act))
        self.fshape[y] = list(self.fshape[a])
        return y

    def detection_postprocess(self, boxes_f, scores_f, anchors, num_classes, max_detections=25,
                              score_threshold=0.4, iou_threshold=0.5, scales=(10.0, 10.0, 5.0, 5.0)):
        """TFLite_Detection_PostProcess (CUSTOM; fast NMS, one class per
        detection): float box encodings [1,N,4], float class scores
        [1,N,C(+1)], constant anchors [N,4] (y, x, h, w) -> boxes, classes,
        scores, num_detections"""
        n = anchors.shape[0]
        a = self.mb.tensor(self._name("anchors"), [n, 4], np.float32, data=anchors.astype(np.float32))
        outs = [self.mb.tensor(self._name("detection_boxes"), [1, max_detections, 4], np.float32),
                self.mb.tensor(self._name("detection_classes"), [1, max_detections], np.float32),
                self.mb.tensor(self._name("detection_scores"), [1, max_detections], np.float32),
                self.mb.tensor(self._name("num_detections"), [1], np.float32)]
        opts = flexbuffer_map(dict(max_detections=int(max_detections), max_classes_per_detection=1,
                                   detections_per_class=100, use_regular_nms=False,
                                   nms_score_threshold=float(score_threshold), nms_iou_threshold=float(iou_threshold),
                                   num_classes=int(num_classes), y_scale=float(scales[0]), x_scale=float(scales[1]),
                                   h_scale=float(scales[2]), w_scale=float(scales[3])))
        self.mb.op("CUSTOM", [boxes_f, scores_f, a], outs, custom="TFLite_Detection_PostProcess",
                   custom_options=opts)
        for t, shp in zip(outs, ([1, max_detections, 4], [1, max_detections], [1, max_detections], [1])):
            self.fshape[t] = shp
        return outs

    def arg_max(self, x, axis=-1, output=np.int32, minimum=False, axis_dtype=np.int32):
        """ARG_MAX (ARG_MIN with minimum) of an 8-bit or float32 tensor over
        `axis` (a constant scalar of axis_dtype): int32 / int64 indices, the
        axis removed"""
        shp = list(self.meta[x][0] if x in self.meta else self.fshape[x])
        at = self.mb.tensor(self._name("axis"), [], axis_dtype, data=np.array(axis, axis_dtype))
        del shp[axis]
        y = self.mb.tensor(self._name("arg_min" if minimum else "arg_max"), shp, output)
        opt = Table().set(0, "b", NP_TO_SCHEMA[np.dtype(output)])
        self.mb.op("ARG_MIN" if minimum else "ARG_MAX", [x, at], [y],
                   OPT["ArgMinOptions" if minimum else "ArgMaxOptions"], opt)
        return y

    def quantize_float(self, xf, scale, zp=None):
        """QUANTIZE float32 -> 8-bit"""
        y = self.act_tensor(self.fshape[xf], scale, self._act_zp() if zp is None else zp)
        self.mb.op("QUANTIZE", [xf], [y], OPT["QuantizeOptions"], Table())
        return y

    # --- the ops of a transformer's LayerNorm and MLP ---------------------------
    def _range_q(self, lo, hi, headroom=1.15):
        """(scale, zero point) covering the real interval [lo, hi] with headroom"""
        qmin, qmax = (-128, 127) if self.dtype == np.int8 else (0, 255)
        lo, hi = min(float(lo), 0.0) * headroom, max(float(hi), 0.0) * headroom
        scale = max(hi - lo, 1e-6) / 255.0
        return float(np.float32(scale)), int(np.clip(qmin - round(lo / scale), qmin, qmax))

    def const(self, values, kind="const"):
        """a constant 8-bit tensor holding the real `values` (its own scale and zero point)"""
        v = np.asarray(values, np.float64)
        scale, zp = self._range_q(v.min(), v.max(), 1.0)
        qmin, qmax = (-128, 127) if self.dtype == np.int8 else (0, 255)
        q = np.clip(np.round(v / scale) + zp, qmin, qmax).astype(self.dtype)
        t = self.mb.tensor(self._name(kind), list(v.shape), self.dtype, scale=[scale], zero_point=[zp], data=q)
        self.meta[t] = (list(v.shape), scale, zp)
        return t

    def const_at(self, values, scale, zp, kind="const"):
        """a constant 8-bit tensor holding the real `values` at a given scale and zero point (saturating)"""
        v = np.asarray(values, np.float64)
        qmin, qmax = (-128, 127) if self.dtype == np.int8 else (0, 255)
        q = np.clip(np.round(v / scale) + zp, qmin, qmax).astype(self.dtype)
        t = self.mb.tensor(self._name(kind), list(v.shape), self.dtype, scale=[float(scale)], zero_point=[int(zp)], data=q)
        self.meta[t] = (list(v.shape), float(scale), int(zp))
        return t

    def _binary(self, kind, options, a, b, scale, zp, act="NONE"):
        shape = [int(d) for d in np.broadcast_shapes(tuple(self.meta[a][0]), tuple(self.meta[b][0]))]
        y = self.act_tensor(shape, float(scale), int(zp))
        self.mb.op(kind, [a, b], [y], OPT[options], act_options(act) if options != "SquaredDifferenceOptions" else Table())
        return y

    def mul(self, a, b, scale, zp, act="NONE"):
        """MUL with numpy broadcasting; b may be a constant (self.const)"""
        return self._binary("MUL", "MulOptions", a, b, scale, zp, act)

    def sub(self, a, b, scale, zp, act="NONE"):
        return self._binary("SUB", "SubOptions", a, b, scale, zp, act)

    def add_q(self, a, b, scale, zp, act="NONE"):
        """ADD with broadcasting and an explicit output quantisation"""
        return self._binary("ADD", "AddOptions", a, b, scale, zp, act)

    def squared_difference(self, a, b, scale, zp):
        return self._binary("SQUARED_DIFFERENCE", "SquaredDifferenceOptions", a, b, scale, zp)

    def mean_last(self, x, keep_dims=True, scale=None, zp=None):
        """MEAN over the last axis; the default output shares the input's
        quantisation (reduce.cc's reference_ops::Mean branch)"""
        shp, s, z = self.meta[x]
        at = self.mb.tensor(self._name("axes"), [1], np.int32, data=np.array([-1], np.int32))
        y = self.act_tensor(list(shp[:-1]) + ([1] if keep_dims else []), s if scale is None else float(scale),
                            z if zp is None else int(zp))
        self.mb.op("MEAN", [x, at], [y], OPT["ReducerOptions"], Table().set(0, "b", int(keep_dims)))
        return y

    def rsqrt(self, x, scale, zp):
        y = self._like(x, scale=float(scale), zp=int(zp))
        self.mb.op("RSQRT", [x], [y])
        return y

    def gelu(self, x, approximate=False):
        """GELU at the input's scale; the zero point leaves room for the minimum, -0.17"""
        _, s, _ = self.meta[x]
        qmin = -128 if self.dtype == np.int8 else 0
        y = self._like(x, zp=min(qmin + int(np.ceil(0.17 / s)), qmin + 128))
        self.mb.op("GELU", [x], [y], OPT["GeluOptions"], Table().set(0, "b", int(approximate)))
        return y

    def layer_norm(self, x, eps=1e-6):
        """The ten ops a converter makes of LayerNormalization over the last axis:
        m = MEAN(x), d = SQUARED_DIFFERENCE(x, m), v = MEAN(d), e = ADD(v, eps),
        r = RSQRT(e), g = MUL(r, gamma), a = MUL(x, g), b = MUL(m, g),
        c = SUB(beta, b), y = ADD(a, c).  gamma ~ U(0.5, 1.5) and beta ~ N(0, 0.3)
        per channel.  The scale of every intermediate comes from a float64 pass
        over seeded calibration rows (spreads of 24 to 100 input LSBs around the
        zero point), so that none of them saturates on such inputs; the
        non-negative ones (d, v, e, r, g) sit at the bottom of the range, which
        also keeps RSQRT's input at or above its zero point."""
        assert self.dtype == np.int8, "layer_norm: int8 graphs only (SQUARED_DIFFERENCE and RSQRT are int8 ops)"
        shp, s_x, z_x = self.meta[x]
        C = shp[-1]
        gamma = self.rng.uniform(0.5, 1.5, C)
        beta = self.rng.normal(0.0, 0.3, C)
        cal = np.random.default_rng(1000 + C)
        spread = np.exp(np.linspace(np.log(24.0), np.log(100.0), 64))[:, None]
        X = s_x * np.clip(np.round(cal.normal(0.0, 1.0, (64, C)) * spread / 2.0 + cal.normal(0.0, 10.0, (64, 1))),
                          -128 - z_x, 127 - z_x)
        M = X.mean(-1, keepdims=True)
        D = (X - M) ** 2
        V = D.mean(-1, keepdims=True)
        E = V + eps
        R = 1.0 / np.sqrt(E)
        G = R * gamma
        A, B = X * G, M * G
        Cc = beta - B
        Y = A + Cc
        q = lambda t: self._range_q(t.min(), t.max())
        m = self.mean_last(x)
        # squared_difference.cc wants (2 max(s_x, s_m))^2 / (2^14 s_d) < 1 (a constant row has no spread)
        d = self.squared_difference(x, m, max(q(D)[0], 1.01 * (2.0 * s_x) ** 2 / 16384.0), -128)
        v = self.mean_last(d, scale=q(V)[0], zp=-128)
        e = self.add_q(v, self.const([eps], "eps"), q(E)[0], -128)
        # 1 / sqrt reaches its maximum on the smallest variance; twice the calibrated one leaves room
        r = self.rsqrt(e, 2.0 * q(R)[0], -128)
        g = self.mul(r, self.const(gamma, "gamma"), 2.0 * q(G)[0], -128)
        a = self.mul(x, g, *q(2.0 * A))
        b = self.mul(m, g, *q(2.0 * B))
        c = self.sub(self.const(beta, "beta"), b, *q(2.0 * Cc))
        return self.add_q(a, c, *q(Y))

    def mlp(self, x, hidden, residual=None):
        """FULLY_CONNECTED -> GELU -> FULLY_CONNECTED -> ADD with the input (or with `residual`)"""
        c = self.meta[x][0][-1]
        h = self.gelu(self.fully_connected(x, hidden, keep_num_dims=True))
        return self.add(self.fully_connected(h, c, keep_num_dims=True), x if residual is None else residual)

    def build(self):
        return self.mb.build()


class FGraph(_ReindexOps):
    """Float graph builder with QGraph's method names: a TFLite fp16 model
    (post-training float16 quantization) - float32 activations, every
    constant stored as float16 behind a DEQUANTIZE op, float32 compute.
    Weights are He-initialised so activations stay O(1) through ReLU6.

    hybrid = "symmetric" | "asymmetric" builds the converter's dynamic-range
    form instead: every constant a plain float32 tensor (no DEQUANTIZE), every
    FULLY_CONNECTED with int8 weights (fully_connected's `hybrid`).

    hybrid_conv = "per_channel" | "per_tensor" makes the graph dynamic-range
    too (float32 constants, no DEQUANTIZE) and gives CONV_2D and
    DEPTHWISE_CONV_2D int8 filters (conv's / dwconv's `hybrid`): ws = max|w| /
    127 over each output channel (quantized_dimension 0, 3 for depthwise) or
    over the whole filter, zero points 0, a plain float32 bias.  A depthwise
    filter is per-channel under either graph setting.  Filters of fewer than
    hybrid_min_elements elements stay float32, as the converter leaves small
    weights alone (1024, restated from memory of the converter; 0 quantises
    every filter)."""

    def __init__(self, seed=0, name="model", hybrid=None, hybrid_conv=None, hybrid_min_elements=1024):
        assert hybrid in (None, "symmetric", "asymmetric"), hybrid
        assert hybrid_conv in (None, "per_channel", "per_tensor"), hybrid_conv
        self.hybrid = hybrid
        self.hybrid_conv = hybrid_conv
        self.hybrid_min_elements = hybrid_min_elements
        self.dtype = np.dtype(np.float16)
        self.rng = np.random.default_rng(seed)
        self.mb = ModelBuilder(name)
        self.n = 0
        self.meta = {}  # tensor -> (shape, None, None)

    def _name(self, kind):
        self.n += 1
        return "%s_%d" % (kind, self.n)

    def _act(self, shape, kind="act"):
        t = self.mb.tensor(self._name(kind), list(shape), np.float32)
        self.meta[t] = (list(shape), None, None)
        return t

    def _const(self, values, kind):
        """float16 constant + DEQUANTIZE -> float32 tensor (a dynamic-range graph: a float32 constant)"""
        v = np.asarray(values, np.float32)
        if self.hybrid or self.hybrid_conv:
            return self.mb.tensor(self._name(kind), list(v.shape), np.float32, data=v)
        c = self.mb.tensor(self._name(kind + "_fp16"), list(v.shape), np.float16, data=v.astype(np.float16))
        y = self.mb.tensor(self._name(kind), list(v.shape), np.float32)
        self.mb.op("DEQUANTIZE", [c], [y], OPT["DequantizeOptions"], Table())
        return y

    def input(self, shape, scale=None, zp=None, dtype=None):
        """a float32 model input; dtype np.int32 / np.int64: an index tensor (token ids)"""
        if dtype is not None:
            t = self.mb.tensor(self._name("input"), list(shape), dtype)
            self.meta[t] = (list(shape), None, None)
        else:
            t = self._act(shape, "input")
        self.mb.inputs.append(t)
        return t

    def output(self, t):
        self.mb.outputs.append(t)

    def _hybrid_filter(self, wv, bv, mode, axis, kind):
        """int8 filter tensor (scales over `axis`, the output channels, or one for the whole filter) and float32 bias"""
        wv = np.asarray(wv, np.float32)
        if mode == "per_channel":
            red = tuple(a for a in range(wv.ndim) if a != axis)
            ws = (np.abs(wv).max(axis=red, keepdims=True).astype(np.float32) / np.float32(127.0)).astype(np.float32)
            ws[ws == 0] = 1.0
            scale = [float(v) for v in ws.reshape(-1)]
        else:
            ws = np.float32(np.float32(np.abs(wv).max()) / np.float32(127.0)) or np.float32(1.0)
            scale = [float(ws)]
        wq = np.clip(np.round(wv / ws), -127, 127).astype(np.int8)
        wt = self.mb.tensor(self._name(kind), list(wv.shape), np.int8, scale=scale, zero_point=[0] * len(scale),
                            qdim=axis if mode == "per_channel" else 0, data=wq)
        bt = self.mb.tensor(self._name(kind.replace("weights", "bias")), [wv.shape[axis]], np.float32,
                            data=np.asarray(bv, np.float32))
        return wt, bt

    def _conv_mode(self, hybrid, elements, depthwise):
        assert hybrid in (None, "per_channel", "per_tensor"), hybrid
        if hybrid:
            return hybrid  # the call's own choice, whatever the size
        if not self.hybrid_conv or elements < self.hybrid_min_elements:
            return None
        return "per_channel" if depthwise else self.hybrid_conv

    def conv(self, x, out_c, k=1, stride=1, act="RELU6", padding="SAME", dilation=1, out_scale=None,
             bias_offset_lsb=0, hybrid=None):
        """hybrid = "per_channel" | "per_tensor" (default: the graph's hybrid_conv above
        hybrid_min_elements): an int8 filter, see the class"""
        b, h, w, c = self.meta[x][0]
        K = k * k * c
        mode = self._conv_mode(hybrid, out_c * K, False)
        wv = self.rng.normal(0, np.sqrt(2.0 / K), (out_c, k, k, c))
        bv = self.rng.normal(0, 0.05, out_c) + (bias_offset_lsb * 0.05 if bias_offset_lsb else 0)
        if mode:
            wt, bt = self._hybrid_filter(wv, bv, mode, 0, "weights")
        else:
            wt = self._const(wv, "weights")
            bt = self._const(bv, "bias")
        eff = (k - 1) * dilation + 1
        oh = (h + stride - 1) // stride if padding == "SAME" else (h + stride - eff) // stride
        ow = (w + stride - 1) // stride if padding == "SAME" else (w + stride - eff) // stride
        y = self._act([b, oh, ow, out_c])
        self.mb.op("CONV_2D", [x, wt, bt], [y], OPT["Conv2DOptions"], conv_options(padding, stride, act, dilation))
        return y

    def dwconv(self, x, k=3, stride=1, act="RELU6", padding="SAME", dm=1, dilation=1, hybrid=None):
        """hybrid: as conv's; scales over dimension 3"""
        b, h, w, c = self.meta[x][0]
        out_c = c * dm
        mode = self._conv_mode(hybrid, k * k * out_c, True)
        wv = self.rng.normal(0, np.sqrt(2.0 / (k * k)), (1, k, k, out_c))
        bv = self.rng.normal(0, 0.05, out_c)
        if mode:
            wt, bt = self._hybrid_filter(wv, bv, mode, 3, "dw_weights")
        else:
            wt = self._const(wv, "dw_weights")
            bt = self._const(bv, "dw_bias")
        eff = (k - 1) * dilation + 1
        oh = (h + stride - 1) // stride if padding == "SAME" else (h + stride - eff) // stride
        ow = (w + stride - 1) // stride if padding == "SAME" else (w + stride - eff) // stride
        y = self._act([b, oh, ow, out_c])
        self.mb.op("DEPTHWISE_CONV_2D", [x, wt, bt], [y], OPT["DepthwiseConv2DOptions"],
                   dw_options(padding, stride, act, dm, dilation))
        return y

    def add(self, a, b, act="NONE"):
        y = self._act(self.meta[a][0])
        self.mb.op("ADD", [a, b], [y], OPT["AddOptions"], act_options(act))
        return y

    def mul(self, a, b, act="NONE"):
        y = self._act(self.meta[a][0])
        self.mb.op("MUL", [a, b], [y], OPT["MulOptions"], act_options(act))
        return y

    def _pool(self, kind, x, filt, stride, padding):
        b, h, w, c = self.meta[x][0]
        oh = (h + stride - filt[0]) // stride if padding == "VALID" else (h + stride - 1) // stride
        ow = (w + stride - filt[1]) // stride if padding == "VALID" else (w + stride - 1) // stride
        y = self._act([b, oh, ow, c])
        self.mb.op(kind, [x], [y], OPT["Pool2DOptions"], pool_options(padding, stride, filt))
        return y

    def avgpool(self, x, filt, stride=1, padding="VALID"):
        return self._pool("AVERAGE_POOL_2D", x, filt, stride, padding)

    def maxpool(self, x, filt, stride, padding="SAME"):
        return self._pool("MAX_POOL_2D", x, filt, stride, padding)

    def reshape(self, x, shape):
        st = self.mb.tensor(self._name("shape"), [len(shape)], np.int32, data=np.array(shape, np.int32))
        y = self._act(list(shape))
        self.mb.op("RESHAPE", [x, st], [y], OPT["ReshapeOptions"], Table().set(0, "o", Vec("i", list(shape))))
        return y

    def fully_connected(self, x, units, act="NONE", keep_num_dims=False, gain=1.0, hybrid=None):
        """`gain` scales the weights' standard deviation (an attention block's 1 / sqrt(D) folded into Q).
        hybrid = "symmetric" | "asymmetric" (default: the graph's): int8 weights with ws = max|w| / 127
        and zero point 0, a plain float32 bias constant, asymmetric_quantize_inputs (slot 3) when asymmetric"""
        hybrid = hybrid or self.hybrid
        assert hybrid in (None, "symmetric", "asymmetric"), hybrid
        shp = self.meta[x][0]
        depth = shp[-1]
        rows = int(np.prod(shp)) // depth
        w = self.rng.normal(0, gain * np.sqrt(1.0 / depth), (units, depth))
        b = self.rng.normal(0, 0.05, units)
        if hybrid:
            w = w.astype(np.float32)
            ws = float(np.float32(np.abs(w).max()) / np.float32(127.0)) or 1.0
            wq = np.clip(np.round(w / np.float32(ws)), -127, 127).astype(np.int8)
            wt = self.mb.tensor(self._name("fc_weights"), [units, depth], np.int8, scale=[ws], zero_point=[0], data=wq)
            bt = self.mb.tensor(self._name("fc_bias"), [units], np.float32, data=b.astype(np.float32))
        else:
            wt = self._const(w, "fc_weights")
            bt = self._const(b, "fc_bias")
        y = self._act(list(shp[:-1]) + [units] if keep_num_dims else [rows, units])
        opt = act_options(act)
        if keep_num_dims:
            opt.set(2, "b", 1)
        if hybrid == "asymmetric":
            opt.set(3, "b", 1)
        self.mb.op("FULLY_CONNECTED", [x, wt, bt], [y], OPT["FullyConnectedOptions"], opt)
        return y

    def batch_matmul(self, a, b, adj_x=False, adj_y=False, out_scale=None, out_zp=None):
        shape, _ = _bmm_shape(self.meta[a][0], self.meta[b][0], adj_x, adj_y)
        y = self._act(shape)
        self.mb.op("BATCH_MATMUL", [a, b], [y], OPT["BatchMatMulOptions"], bmm_options(adj_x, adj_y))
        return y

    def concat(self, xs, axis=3):
        shp = list(self.meta[xs[0]][0])
        shp[axis] = sum(self.meta[t][0][axis] for t in xs)
        y = self._act(shp)
        self.mb.op("CONCATENATION", list(xs), [y], OPT["ConcatenationOptions"], Table().set(0, "i", axis))
        return y

    def logistic(self, x):
        y = self._act(self.meta[x][0])
        self.mb.op("LOGISTIC", [x], [y])
        return y

    def tanh(self, x):
        y = self._act(self.meta[x][0])
        self.mb.op("TANH", [x], [y])
        return y

    def softmax(self, x, beta=1.0):
        y = self._act(self.meta[x][0])
        self.mb.op("SOFTMAX", [x], [y], OPT["SoftmaxOptions"], Table().set(0, "f", float(beta)))
        return y

    def relu(self, x, kind="RELU"):
        y = self._act(self.meta[x][0])
        self.mb.op(kind, [x], [y])
        return y

    # --- the ops of a transformer's LayerNorm and MLP (QGraph's names) ---------
    def const(self, values, kind="const"):
        v = np.asarray(values, np.float32)
        t = self._const(v, kind)
        self.meta[t] = (list(v.shape), None, None)
        return t

    def _binary(self, kind, options, a, b, act="NONE"):
        shape = [int(d) for d in np.broadcast_shapes(tuple(self.meta[a][0]), tuple(self.meta[b][0]))]
        y = self._act(shape)
        self.mb.op(kind, [a, b], [y], OPT[options], act_options(act) if options != "SquaredDifferenceOptions" else Table())
        return y

    def sub(self, a, b, act="NONE"):
        return self._binary("SUB", "SubOptions", a, b, act)

    def squared_difference(self, a, b):
        return self._binary("SQUARED_DIFFERENCE", "SquaredDifferenceOptions", a, b)

    def mean_last(self, x, keep_dims=True):
        shp = self.meta[x][0]
        at = self.mb.tensor(self._name("axes"), [1], np.int32, data=np.array([-1], np.int32))
        y = self._act(list(shp[:-1]) + ([1] if keep_dims else []))
        self.mb.op("MEAN", [x, at], [y], OPT["ReducerOptions"], Table().set(0, "b", int(keep_dims)))
        return y

    def rsqrt(self, x):
        y = self._act(self.meta[x][0])
        self.mb.op("RSQRT", [x], [y])
        return y

    def gelu(self, x, approximate=False):
        y = self._act(self.meta[x][0])
        self.mb.op("GELU", [x], [y], OPT["GeluOptions"], Table().set(0, "b", int(approximate)))
        return y

    def layer_norm(self, x, eps=1e-6):
        """QGraph.layer_norm's ten ops in float32"""
        C = self.meta[x][0][-1]
        gamma = self.const(self.rng.uniform(0.5, 1.5, C), "gamma")
        beta = self.const(self.rng.normal(0.0, 0.3, C), "beta")
        m = self.mean_last(x)
        v = self.mean_last(self.squared_difference(x, m))
        r = self.rsqrt(self._binary("ADD", "AddOptions", v, self.const([eps], "eps")))
        g = self._binary("MUL", "MulOptions", r, gamma)
        a = self._binary("MUL", "MulOptions", x, g)
        b = self._binary("MUL", "MulOptions", m, g)
        return self._binary("ADD", "AddOptions", a, self.sub(beta, b))

    def mlp(self, x, hidden, residual=None):
        c = self.meta[x][0][-1]
        h = self.gelu(self.fully_connected(x, hidden, keep_num_dims=True))
        return self.add(self.fully_connected(h, c, keep_num_dims=True), x if residual is None else residual)

    def build(self):
        return self.mb.build()


def _graph(dtype, seed, name, hybrid_conv=None, hybrid_min_elements=1024):
    """QGraph for 8-bit models, FGraph for fp16-weight float models and, with
    hybrid_conv, for the dynamic-range float32 CNN"""
    if hybrid_conv:
        assert np.dtype(dtype) == np.dtype(np.float32), "hybrid_conv is a form of the float32 model"
        return FGraph(seed, name + "_hybrid", hybrid_conv=hybrid_conv, hybrid_min_elements=hybrid_min_elements)
    if np.dtype(dtype) == np.float16:
        return FGraph(seed, name)
    return QGraph(dtype, seed, name)


# ---------------------------------------------------------------------------
# BASELINE models
# ---------------------------------------------------------------------------
MNV2_BLOCKS = [(1, 16, 1, 1), (6, 24, 2, 2), (6, 32, 3, 2), (6, 64, 4, 2), (6, 96, 3, 1),
               (6, 160, 3, 2), (6, 320, 1, 1)]


def mobilenet_v2(dtype=np.int8, seed=0, size=224, batch=1, classes=1001, width=1.0, hybrid_conv=None,
                 hybrid_min_elements=1024):
    """MobileNetV2-1.0 with the topology of mobilenet_v2_1.0_224_quant.tflite
    (65 ops: 36 CONV_2D, 17 DEPTHWISE_CONV_2D, 10 ADD, AVERAGE_POOL_2D, RESHAPE).
    dtype float32 with hybrid_conv ("per_channel" | "per_tensor") builds the
    dynamic-range CNN (FGraph): float32 constants, int8 filters."""
    g = _graph(dtype, seed, "mobilenet_v2_%s" % np.dtype(dtype).name, hybrid_conv, hybrid_min_elements)
    ch = lambda c: max(8, int(c * width + 4) // 8 * 8)
    x = g.input([batch, size, size, 3])
    x = g.conv(x, ch(32), k=3, stride=2)
    c_in = ch(32)
    for t, c, n, s in MNV2_BLOCKS:
        for i in range(n):
            inp = x
            stride = s if i == 0 else 1
            h = x
            if t != 1:
                h = g.conv(h, c_in * t, k=1)
            h = g.dwconv(h, k=3, stride=stride)
            h = g.conv(h, ch(c), k=1, act="NONE")
            if stride == 1 and c_in == ch(c):
                h = g.add(h, inp)
            x = h
            c_in = ch(c)
    x = g.conv(x, 1280 if width <= 1.0 else ch(1280), k=1)
    k = size // 32
    x = g.avgpool(x, (k, k))
    x = g.conv(x, classes, k=1, act="NONE")
    x = g.reshape(x, [batch, classes])
    g.output(x)
    return g.build()


def mobilenet_v1(dtype=np.int8, seed=0, size=224, batch=1, classes=1001, hybrid_conv=None, hybrid_min_elements=1024):
    """MobileNetV1-1.0 (config C1): conv + 13 depthwise-separable blocks.
    hybrid_conv: the dynamic-range CNN, as mobilenet_v2's."""
    g = _graph(dtype, seed, "mobilenet_v1_%s" % np.dtype(dtype).name, hybrid_conv, hybrid_min_elements)
    x = g.input([batch, size, size, 3])
    x = g.conv(x, 32, k=3, stride=2)
    for c, s in [(64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2), (512, 1), (512, 1),
                 (512, 1), (512, 1), (512, 1), (1024, 2), (1024, 1)]:
        x = g.dwconv(x, stride=s)
        x = g.conv(x, c, k=1)
    k = size // 32
    x = g.avgpool(x, (k, k))
    x = g.conv(x, classes, k=1, act="NONE")
    x = g.reshape(x, [batch, classes])
    g.output(x)
    return g.build()


def shufflenet_v1(dtype=np.int8, seed=5, size=224, groups=3, width=1.0, batch=1, classes=1000, repeats=(3, 7, 3)):
    """ShuffleNet-v1 (Zhang et al. 2018, table 1; 240 / 480 / 960 channels at
    groups=3, width 1.0).  A unit is grouped 1x1 CONV_2D -> channel shuffle
    (RESHAPE - TRANSPOSE - RESHAPE) -> depthwise 3x3 -> grouped 1x1 CONV_2D,
    joined to its input by ADD (stride 1) or, after a 3x3 stride-2 average
    pool of the input, by CONCATENATION (stride 2).  The very first grouped
    layer is dense, as in the paper (its input has 8 * groups channels)."""
    g = QGraph(dtype, seed, "shufflenet_v1_g%d_%s" % (groups, np.dtype(dtype).name))
    q = 4 * groups  # stage widths: the bottleneck (a quarter) splits into `groups`
    stem = 8 * groups
    x = g.input([batch, size, size, 3])
    x = g.conv(x, stem, k=3, stride=2)
    x = g.maxpool(x, (3, 3), 2)
    c_in = stem
    for stage, n in enumerate(repeats):
        c_out = max(q, int(80 * groups * width * (1 << stage)) // q * q)
        for i in range(n + 1):
            stride = 2 if i == 0 else 1
            mid = c_out // 4
            branch_out = c_out - c_in if stride == 2 else c_out
            _, h, w, _ = g.meta[x][0]
            y = g.conv(x, mid, k=1, groups=1 if (stage == 0 and i == 0) else groups)
            y = g.reshape(y, [batch, h, w, groups, mid // groups])
            y = g.transpose(y, (0, 1, 2, 4, 3))
            y = g.reshape(y, [batch, h, w, mid])
            y = g.dwconv(y, k=3, stride=stride, act="NONE")
            y = g.conv(y, branch_out, k=1, act="NONE", groups=groups)
            if stride == 2:
                x = g.relu(g.concat([g.avgpool(x, (3, 3), 2, "SAME"), y], axis=3))
            else:
                x = g.add(y, x, act="RELU")
            c_in = c_out
    _, h, w, _ = g.meta[x][0]
    x = g.avgpool(x, (h, w))
    x = g.conv(x, classes, k=1, act="NONE")
    g.output(g.reshape(x, [batch, classes]))
    return g.build()


# ---------------------------------------------------------------------------
# BASELINE C3 mix: detection / segmentation / pose heads on MobileNet trunks
# (synthetic weights, 224x224 inputs - "synthetic 224x224 batches", §8(d))
# ---------------------------------------------------------------------------
MASKED = -10000.0  # what an attention mask adds to the score of a key that must not be seen


def _attention(g, x, heads, residual=None, bias=None):
    """One multi-head self-attention block on x [B, T, C] (no LayerNorm): Q, K, V
    projections, per-head softmax(Q K^T / sqrt(D)) V, output projection,
    residual ADD (with x, or with `residual`: a pre-norm block's input).
    `bias`: a tensor that broadcasts to the scores [B, H, T, T] (a padding mask
    [B, 1, 1, T], a causal mask [1, 1, T, T], a position bias [1, H, T, T]), or
    a function (g, scores) -> such a tensor; it is ADDed to the scores before
    the SOFTMAX, and in the 8-bit model the sum keeps the scores' quantisation,
    so a masked key saturates at the bottom of the range.
    The float model's 1 / sqrt(D) leaves no op: it is folded
    into the Q projection (its output scale, so its filter scale, is the
    input's over sqrt(D); the fp16 model scales the Q weights), and the scores'
    scale then stands for Q K^T / sqrt(D)."""
    b, t, c = g.meta[x][0]
    d = c // heads
    assert d * heads == c, "heads must divide dim"
    quant = isinstance(g, QGraph)
    s_in = g.meta[x][1]
    if quant:
        q = g.fully_connected(x, c, keep_num_dims=True, out_scale=s_in / np.sqrt(d))
    else:
        q = g.fully_connected(x, c, keep_num_dims=True, gain=1.0 / np.sqrt(d))
    k = g.fully_connected(x, c, keep_num_dims=True)
    v = g.fully_connected(x, c, keep_num_dims=True)
    q, k, v = [g.transpose(g.reshape(z, [b, t, heads, d]), (0, 2, 1, 3)) for z in (q, k, v)]
    scores = g.batch_matmul(q, k, adj_y=True)            # [B, H, T, T]
    if bias is not None:
        bt = bias(g, scores) if callable(bias) else bias
        scores = g.add_q(scores, bt, g.meta[scores][1], g.meta[scores][2]) if quant else g.add(scores, bt)
    p = g.softmax(scores, beta=1.0)                      # scale 1 / 256, zero point -128
    # a row of P sums to ~256 LSBs, so at V's scale the context is V's weighted mean
    ctx = g.batch_matmul(p, v, out_scale=g.meta[v][1] if quant else None)  # [B, H, T, D]
    ctx = g.reshape(g.transpose(ctx, (0, 2, 1, 3)), [b, t, c])
    y = g.fully_connected(ctx, c, keep_num_dims=True)
    return g.add(y, x if residual is None else residual)


def _mask_const(g, values, kind):
    """an additive attention mask of 0 / MASKED as a constant: 8-bit at scale -MASKED / 255 with 0 at the top of
    the range, so the two values are the range's two ends"""
    if isinstance(g, QGraph):
        return g.const_at(values, -MASKED / 255.0, 127 if g.dtype == np.int8 else 255, kind)
    return g.const(values, kind)


def _attention_bias(kind, tokens, heads):
    """attention_block's attention_bias as _attention's bias function"""
    if kind == "causal":
        # key j is seen from row i when j <= i
        return lambda g, scores: _mask_const(g, np.triu(np.full((1, 1, tokens, tokens), MASKED), 1), "causal_mask")

    def relative(g, scores):
        # drawn over the whole 8-bit range at the scores' quantisation (Swin, T5: a learnt table, gathered at
        # conversion time)
        if not isinstance(g, QGraph):
            return g.const(g.rng.normal(0.0, 1.0, (1, heads, tokens, tokens)), "position_bias")
        _, s, z = g.meta[scores]
        qmin, qmax = (-128, 127) if g.dtype == np.int8 else (0, 255)
        q = g.rng.integers(qmin, qmax + 1, (1, heads, tokens, tokens))
        return g.const_at((q - z) * s, s, z, "position_bias")
    assert kind == "relative", kind
    return relative


def attention_block(dtype=np.int8, seed=6, tokens=196, dim=192, heads=3, batch=1, hybrid=None, attention_bias=None):
    """attention_bias: None, "causal" (a constant [1, 1, T, T] mask, 0 on and below the diagonal and MASKED above
    it) or "relative" (a constant [1, H, T, T] position bias), ADDed to the scores before the SOFTMAX.
    One self-attention block on [batch, tokens, dim]: three FULLY_CONNECTED
    (keep_num_dims), RESHAPE / TRANSPOSE to [batch, heads, tokens, dim / heads],
    BATCH_MATMUL(adj_y) -> SOFTMAX -> BATCH_MATMUL, TRANSPOSE / RESHAPE back,
    FULLY_CONNECTED, ADD with the input.  dtype float32 (or float16) builds the
    fp16-constant float model, or with `hybrid` ("symmetric" | "asymmetric") the
    dynamic-range one (FGraph).  No LayerNorm: encoder_block has it."""
    assert hybrid is None or np.dtype(dtype) == np.dtype(np.float32), "hybrid is a form of the float32 model"
    if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.float16)):
        g = FGraph(seed, "attention_block_f32" + ("_hybrid" if hybrid else ""), hybrid=hybrid)
    else:
        g = QGraph(dtype, seed, "attention_block_%s" % np.dtype(dtype).name)
    x = g.input([batch, tokens, dim], scale=0.05)
    g.output(_attention(g, x, heads, bias=_attention_bias(attention_bias, tokens, heads) if attention_bias else None))
    return g.build()


def _encoder(g, x, heads, hidden, layer_norm=True, mlp=True, bias=None):
    """The pre-norm transformer block on x [B, T, C]: x + attention(LN(x)),
    then the same around the MLP (FULLY_CONNECTED -> GELU -> FULLY_CONNECTED).
    `bias`: _attention's."""
    y = _attention(g, g.layer_norm(x) if layer_norm else x, heads, residual=x, bias=bias)
    if mlp:
        y = g.mlp(g.layer_norm(y) if layer_norm else y, hidden, residual=y)
    return y


def encoder_block(dtype=np.int8, seed=8, tokens=196, dim=192, heads=3, hidden=768, batch=1, hybrid=None):
    """One pre-norm transformer encoder block on [batch, tokens, dim]:
    LayerNorm (the converter's ten ops, see QGraph.layer_norm) -> attention
    (attention_block's) -> LayerNorm -> MLP (FULLY_CONNECTED to `hidden`, GELU,
    FULLY_CONNECTED back), with the residual ADDs.  dtype float32 (or float16)
    builds the fp16-constant float model, or with `hybrid` ("symmetric" |
    "asymmetric") the dynamic-range one (FGraph)."""
    assert hybrid is None or np.dtype(dtype) == np.dtype(np.float32), "hybrid is a form of the float32 model"
    if np.dtype(dtype) in (np.dtype(np.float32), np.dtype(np.float16)):
        g = FGraph(seed, "encoder_block_f32" + ("_hybrid" if hybrid else ""), hybrid=hybrid)
    else:
        g = QGraph(dtype, seed, "encoder_block_%s" % np.dtype(dtype).name)
    x = g.input([batch, tokens, dim], scale=0.05)
    g.output(_encoder(g, x, heads, hidden))
    return g.build()


def vit_tiny(dtype=np.int8, seed=7, size=224, dim=192, heads=3, blocks=2, batch=1, layer_norm=False, mlp=False,
             hybrid=None, hybrid_conv=None, hybrid_min_elements=1024):
    """ViT-Tiny's front: a 16 x 16 stride-16 patch CONV_2D, RESHAPE to tokens
    [batch, (size / 16)^2, dim] and `blocks` attention blocks; with layer_norm
    / mlp, pre-norm encoder blocks (encoder_block's, hidden = 4 dim).  No
    class token and no position embedding.  dtype float32 with `hybrid`
    ("symmetric" | "asymmetric") builds the dynamic-range float model: a float32
    patch conv, hybrid FULLY_CONNECTEDs; with hybrid_conv ("per_channel" |
    "per_tensor") beside it the patch conv is hybrid too."""
    assert not hybrid_conv or hybrid, "hybrid_conv goes with hybrid"
    if hybrid:
        assert np.dtype(dtype) == np.dtype(np.float32), "hybrid is a form of the float32 model"
        g = FGraph(seed, "vit_tiny_f32_hybrid", hybrid=hybrid, hybrid_conv=hybrid_conv,
                   hybrid_min_elements=hybrid_min_elements)
    else:
        g = QGraph(dtype, seed, "vit_tiny_%s" % np.dtype(dtype).name)
    x = g.input([batch, size, size, 3], scale=0.05)
    y = g.conv(x, dim, k=16, stride=16, act="NONE", padding="VALID")
    n = (size // 16) ** 2
    y = g.reshape(y, [batch, n, dim])
    for _ in range(blocks):
        y = _encoder(g, y, heads, 4 * dim, layer_norm, mlp) if (layer_norm or mlp) else _attention(g, y, heads)
    g.output(y)
    return g.build()


def _padding_mask(g, batch, tokens):
    """A BERT attention mask as the converter leaves it: a second int32 input [batch, tokens] (1: a token, 0:
    padding), CAST to float32, SUB (1 - m), MUL by MASKED; in the 8-bit model a QUANTIZE to 8 bits at scale -MASKED /
    255 with 0 at the top of the range; RESHAPE to [batch, 1, 1, tokens].  The float32 ops of the 8-bit model are
    written here by hand (QGraph's SUB / MUL are the 8-bit ones)."""
    m = g.input([batch, tokens], dtype=np.int32)
    f = g.cast(m, np.float32)
    if not isinstance(g, QGraph):
        y = g.mul(g.sub(g.const([1.0], "one"), f), g.const([MASKED], "masked"))
        return g.reshape(y, [batch, 1, 1, tokens])

    def f32(kind, options, a, value, swap):
        c = g.mb.tensor(g._name("mask_const"), [1], np.float32, data=np.array([value], np.float32))
        y = g.mb.tensor(g._name("mask_f32"), [batch, tokens], np.float32)
        g.meta[y] = ([batch, tokens], None, None)
        g.mb.op(kind, [c, a] if swap else [a, c], [y], OPT[options], act_options("NONE"))
        return y
    y = f32("MUL", "MulOptions", f32("SUB", "SubOptions", f, 1.0, True), MASKED, False)
    q = g.act_tensor([batch, tokens], -MASKED / 255.0, 127 if g.dtype == np.int8 else 255)
    g.mb.op("QUANTIZE", [y], [q], OPT["QuantizeOptions"], Table())
    return g.reshape(q, [batch, 1, 1, tokens])


def text_encoder(dtype=np.int8, seed=9, tokens=128, dim=192, heads=3, hidden=768, blocks=2, vocab=1000, classes=2,
                 batch=1, hybrid=None, pooler=False, embedding_lookup=False, mask=False):
    """A BERT-style classifier on token ids [batch, tokens] int32: GATHER of a
    constant [vocab, dim] embedding table (axis 0), ADD of a constant
    [1, tokens, dim] position embedding, LayerNorm, `blocks` pre-norm encoder
    blocks (encoder_block's), STRIDED_SLICE of token 0 and a FULLY_CONNECTED to
    `classes`.  dtype float32 (or float16) builds the fp16-constant float
    model, or with `hybrid` ("symmetric" | "asymmetric") the dynamic-range one;
    the table is then a float32 constant either way (GATHER reads it as it is
    stored).  Keep vocab > 99: the benchmark tool fills int32 inputs with
    0 .. 99.  embedding_lookup: the table is read by EMBEDDING_LOOKUP instead
    of GATHER; pooler: BERT's pooler, FULLY_CONNECTED(dim) -> TANH on token 0 in
    front of the classifier (8-bit: the TANH output at 1 / 128 around the
    middle of the range); mask: a second int32 input [batch, tokens], 1 for a
    token and 0 for padding, turned into an additive mask (_padding_mask) that
    every block ADDs to its attention scores."""
    assert hybrid is None or np.dtype(dtype) == np.dtype(np.float32), "hybrid is a form of the float32 model"
    quant = np.dtype(dtype) not in (np.dtype(np.float32), np.dtype(np.float16))
    if quant:
        g = QGraph(dtype, seed, "text_encoder_%s" % np.dtype(dtype).name)
    else:
        g = FGraph(seed, "text_encoder_f32" + ("_hybrid" if hybrid else ""), hybrid=hybrid)
    ids = g.input([batch, tokens], dtype=np.int32)
    bias = _padding_mask(g, batch, tokens) if mask else None
    table = g.rng.normal(0.0, 1.0, (vocab, dim))
    if quant:
        tab = g.const(table, "embedding")
    else:
        tab = g.mb.tensor(g._name("embedding"), [vocab, dim], np.float32, data=table.astype(np.float32))
        g.meta[tab] = ([vocab, dim], None, None)
    y = g.embedding_lookup(ids, tab) if embedding_lookup else g.gather(tab, ids, axis=0)
    y = g.add(y, g.const(g.rng.normal(0.0, 0.5, (1, tokens, dim)), "position"))
    y = g.layer_norm(y)
    for _ in range(blocks):
        y = _encoder(g, y, heads, hidden, bias=bias)
    y = g.strided_slice(y, [0, 0, 0], [0, 1, 0], [1, 1, 1], begin_mask=0b101, end_mask=0b101, shrink_axis_mask=0b010)
    if pooler:
        y = g.tanh(g.fully_connected(y, dim))
    g.output(g.fully_connected(y, classes))
    return g.build()


def _mnv2_trunk(g, x, out_stride=32, tap_expansion_at=None):
    """MobileNetV2 feature extractor.  out_stride 16 turns the last stride-2
    stage into stride 1 with dilation 2 (DeepLab).  Returns (features, taps):
    taps["expansion"] = the 1x1 expansion output of block `tap_expansion_at`
    (SSD's 'layer_15/expansion_output')."""
    x = g.conv(x, 32, k=3, stride=2)
    c_in, os_now, dil, taps, blk = 32, 2, 1, {}, 0
    for t, c, n, s in MNV2_BLOCKS:
        for i in range(n):
            inp, stride = x, (s if i == 0 else 1)
            if stride == 2 and os_now >= out_stride:
                stride, dil = 1, dil * 2
            elif stride == 2:
                os_now *= 2
            h = x
            if t != 1:
                h = g.conv(h, c_in * t, k=1)
                if blk == tap_expansion_at:
                    taps["expansion"] = h
            h = g.dwconv(h, k=3, stride=stride, dilation=dil)
            h = g.conv(h, c, k=1, act="NONE")
            if stride == 1 and c_in == c:
                h = g.add(h, inp)
            x, c_in, blk = h, c, blk + 1
    return x, taps


def ssd_anchors(maps, min_scale=0.2, max_scale=0.95):
    """normalised (ycenter, xcenter, h, w) for SSD feature maps [(h, w,
    anchors per cell)], cell-major then anchor, as the predictors' RESHAPE
    lays them out; scales spread linearly over the maps, aspect ratios cycled
    (TF object-detection API's multiple-grid anchor generator, simplified)"""
    ratios = (1.0, 2.0, 0.5, 3.0, 1.0 / 3.0, 1.0)
    out = []
    for i, (h, w, per_cell) in enumerate(maps):
        scale = min_scale + (max_scale - min_scale) * i / max(1, len(maps) - 1)
        for y in range(h):
            for x in range(w):
                for a in range(per_cell):
                    r = ratios[a % len(ratios)]
                    s = scale * (1.15 if a == len(ratios) - 1 else 1.0)
                    out.append(((y + 0.5) / h, (x + 0.5) / w, s / np.sqrt(r), s * np.sqrt(r)))
    return np.array(out, np.float32)


def ssd_mobilenet_v2(dtype=np.int8, seed=1, size=224, batch=1, classes=91, postprocess=False):
    """SSD-MobileNetV2 (TF object-detection API layout): feature maps at
    layer_15/expansion_output (14x14x576) and the 1280-channel head (7x7),
    four extra 1x1 -> 3x3 s2 feature layers, 1x1 box / class predictors,
    RESHAPE + CONCATENATION of all anchors, LOGISTIC class scores.  By
    default the TFLite_Detection_PostProcess custom op is left out: outputs
    are box encodings [1,N,4] and class scores [1,N,classes].  postprocess:
    the real model's tail - DEQUANTIZE of both, then the custom op over
    ssd_anchors (class 0 is the background; 10 detections)."""
    g = _graph(dtype, seed, "ssd_mobilenet_v2_%s" % np.dtype(dtype).name)
    x = g.input([batch, size, size, 3])
    feat, taps = _mnv2_trunk(g, x, tap_expansion_at=13)
    maps = [taps["expansion"], g.conv(feat, 1280, k=1)]
    y = maps[-1]
    for c1, c3 in ((256, 512), (128, 256), (128, 256), (64, 128)):
        y = g.conv(g.conv(y, c1, k=1), c3, k=3, stride=2)
        maps.append(y)
    boxes, scores, grid = [], [], []
    for i, m in enumerate(maps):
        b, h, w, _ = g.meta[m][0]
        anchors = 3 if i == 0 else 6
        bx = g.conv(m, anchors * 4, k=1, act="NONE")
        cl = g.conv(m, anchors * classes, k=1, act="NONE")
        boxes.append(g.reshape(bx, [batch, h * w * anchors, 4]))
        scores.append(g.reshape(cl, [batch, h * w * anchors, classes]))
        grid.append((h, w, anchors))
    box_enc = g.concat(boxes, axis=1)
    cls = g.logistic(g.concat(scores, axis=1))
    if not postprocess:
        g.output(box_enc)
        g.output(cls)
        return g.build()
    for o in g.detection_postprocess(g.dequantize(box_enc), g.dequantize(cls), ssd_anchors(grid), classes - 1,
                                     max_detections=10):
        g.output(o)
    return g.build()


def _round_filters(c, width):
    """EfficientNet channel rounding to a multiple of 8"""
    new = max(8, int(c * width + 4) // 8 * 8)
    if new < 0.9 * c * width:
        new += 8
    return new


# EfficientNet-B0 stages: (expand, kernel, stride, channels, repeats)
EFFNET_STAGES = [(1, 3, 1, 16, 1), (6, 3, 2, 24, 2), (6, 5, 2, 40, 2), (6, 3, 2, 80, 3), (6, 5, 1, 112, 3),
                 (6, 5, 2, 192, 4), (6, 3, 1, 320, 1)]


def efficientdet_anchors(size, levels=(3, 4, 5, 6, 7), anchor_scale=4.0):
    """normalised (ycenter, xcenter, h, w) per feature-map cell x 9 anchors,
    in the order the heads' RESHAPE lays them out"""
    out = []
    for lvl in levels:
        stride = 2 ** lvl
        n = -(-size // stride)
        for y in range(n):
            for x in range(n):
                for sc in (1.0, 2 ** (1 / 3), 2 ** (2 / 3)):
                    for rh, rw in ((1.0, 1.0), (1.4, 0.7), (0.7, 1.4)):
                        base = anchor_scale * stride * sc
                        out.append(((y + 0.5) * stride / size, (x + 0.5) * stride / size,
                                    base * rh / size, base * rw / size))
    return np.array(out, np.float32)


def efficientdet_lite2(dtype=np.int8, seed=4, size=448, batch=1, classes=90, fpn_channels=112, fpn_repeats=5,
                       head_repeats=3, max_detections=25, postprocess=True):
    """EfficientDet-Lite2 (BASELINE C4): EfficientNet-Lite2 backbone (width
    1.1, depth 1.2, ReLU6, no squeeze-excite), BiFPN P3-P7 with 112
    channels x 5 cells (sum fusion, separable convs, nearest upsampling,
    3x3/s2 max-pool downsampling), separable-conv class / box heads with 9
    anchors per cell, LOGISTIC scores, and TFLite_Detection_PostProcess
    (CUSTOM) on DEQUANTIZEd boxes / scores - the op the GPU worker cannot
    run, so the model analyzer splits the model there."""
    g = QGraph(dtype, seed, "efficientdet_lite2_%s" % np.dtype(dtype).name)
    x = g.input([batch, size, size, 3])
    y = g.conv(x, 32, k=3, stride=2)
    taps = []
    n_stages = len(EFFNET_STAGES)
    for si, (t, k, s_, c, r) in enumerate(EFFNET_STAGES):
        c = _round_filters(c, 1.1)
        reps = r if si in (0, n_stages - 1) else int(np.ceil(r * 1.2))
        for i in range(reps):
            stride = s_ if i == 0 else 1
            cin = g.meta[y][0][3]
            h = g.conv(y, cin * t, k=1) if t != 1 else y
            h = g.dwconv(h, k=k, stride=stride)
            h = g.conv(h, c, k=1, act="NONE")
            y = g.add(h, y) if stride == 1 and cin == c else h
        if si in (2, 4, 6):  # strides 8, 16, 32
            taps.append(y)
    F = fpn_channels
    p3, p4, p5 = (g.conv(t_, F, k=1, act="NONE") for t_ in taps)
    p6 = g.maxpool(g.conv(taps[2], F, k=1, act="NONE"), (3, 3), 2)
    p7 = g.maxpool(p6, (3, 3), 2)
    feats = [p3, p4, p5, p6, p7]

    def size_of(t):
        return tuple(g.meta[t][0][1:3])

    def sep(t, act="NONE"):
        return g.conv(g.dwconv(t, k=3, act="NONE"), F, k=1, act=act)

    def fuse(*ts):
        acc = ts[0]
        for i, t in enumerate(ts[1:]):
            acc = g.add(acc, t, act="RELU6" if i == len(ts) - 2 else "NONE")
        return sep(acc)

    for _ in range(fpn_repeats):
        td = [None] * 5
        td[4] = feats[4]
        for l in (3, 2, 1):
            td[l] = fuse(feats[l], g.resize(td[l + 1], size_of(feats[l])))
        out = [None] * 5
        out[0] = fuse(feats[0], g.resize(td[1], size_of(feats[0])))
        for l in (1, 2, 3):
            out[l] = fuse(feats[l], td[l], g.maxpool(out[l - 1], (3, 3), 2))
        out[4] = fuse(feats[4], g.maxpool(out[3], (3, 3), 2))
        feats = out

    boxes, scores = [], []
    for f in feats:
        b_, h, w, _ = g.meta[f][0]
        cl, bx = f, f
        for _ in range(head_repeats):
            cl = sep(cl, act="RELU6")
            bx = sep(bx, act="RELU6")
        # class prior: logits around -5.4, scale 4.6 / 60 (a few hundred anchors pass 0.4)
        cl = g.conv(g.dwconv(cl, k=3, act="NONE"), 9 * classes, k=1, act="NONE", out_scale=4.6 / 60,
                    bias_offset_lsb=-70)
        bx = g.conv(g.dwconv(bx, k=3, act="NONE"), 9 * 4, k=1, act="NONE")
        scores.append(g.reshape(cl, [batch, h * w * 9, classes]))
        boxes.append(g.reshape(bx, [batch, h * w * 9, 4]))
    box_enc = g.concat(boxes, axis=1)
    cls = g.logistic(g.concat(scores, axis=1))
    if not postprocess:
        g.output(box_enc)
        g.output(cls)
        return g.build()
    anchors = efficientdet_anchors(size)
    outs = g.detection_postprocess(g.dequantize(box_enc), g.dequantize(cls), anchors, classes,
                                   max_detections=max_detections)
    for o in outs:
        g.output(o)
    return g.build()


def deeplab_v3_mobilenet_v2(dtype=np.int8, seed=2, size=224, batch=1, classes=21, argmax=None):
    """DeepLabV3 with a MobileNetV2 trunk at output stride 16 (dilated last
    stages) and the mobile ASPP: image pooling (global AVERAGE_POOL_2D, 1x1
    conv, RESIZE_BILINEAR back) + a 1x1 branch, CONCATENATION, 1x1
    projection, 1x1 logits, RESIZE_BILINEAR x16 to the input size.
    argmax=np.int32 / np.int64: the model ends in ARG_MAX over the classes
    and its only output is the [batch, size, size] segmentation map."""
    if argmax is not None and np.dtype(argmax) not in (np.dtype(np.int32), np.dtype(np.int64)):
        raise ValueError("argmax must be None, np.int32 or np.int64")
    g = QGraph(dtype, seed, "deeplab_v3_mnv2_%s" % np.dtype(dtype).name)
    x = g.input([batch, size, size, 3])
    feat, _ = _mnv2_trunk(g, x, out_stride=16)
    fh = g.meta[feat][0][1]
    pool = g.conv(g.avgpool(feat, (fh, fh)), 256, k=1, act="RELU")
    pool = g.resize(pool, (fh, fh), bilinear=True, align_corners=True)
    aspp0 = g.conv(feat, 256, k=1, act="RELU")
    y = g.conv(g.concat([pool, aspp0], axis=3), 256, k=1, act="RELU")
    y = g.conv(y, classes, k=1, act="NONE")
    y = g.resize(y, (size, size), bilinear=True, align_corners=True)
    g.output(y if argmax is None else g.arg_max(y, axis=3, output=argmax))
    return g.build()


def posenet_mobilenet_v1(dtype=np.int8, seed=3, size=224, batch=1, keypoints=17):
    """PoseNet (multi-person, MobileNetV1 trunk at output stride 16): heatmap
    (LOGISTIC), offset and forward / backward displacement 1x1 heads."""
    g = QGraph(dtype, seed, "posenet_mnv1_%s" % np.dtype(dtype).name)
    x = g.input([batch, size, size, 3])
    x = g.conv(x, 32, k=3, stride=2)
    os_now, dil = 2, 1
    for c, s in [(64, 1), (128, 2), (128, 1), (256, 2), (256, 1), (512, 2), (512, 1), (512, 1),
                 (512, 1), (512, 1), (512, 1), (1024, 2), (1024, 1)]:
        if s == 2 and os_now >= 16:
            s, dil = 1, dil * 2
        elif s == 2:
            os_now *= 2
        x = g.dwconv(x, stride=s, dilation=dil)
        x = g.conv(x, c, k=1)
    g.output(g.logistic(g.conv(x, keypoints, k=1, act="NONE")))
    g.output(g.conv(x, 2 * keypoints, k=1, act="NONE"))
    g.output(g.conv(x, 2 * (keypoints - 1), k=1, act="NONE"))
    g.output(g.conv(x, 2 * (keypoints - 1), k=1, act="NONE"))
    return g.build()


MIX_C3 = ("mobilenet_v2", "ssd_mobilenet_v2", "deeplab_v3_mobilenet_v2", "posenet_mobilenet_v1")


def int8_from_uint8(model_bytes):
    """Convert a uint8 per-tensor TFLite model to int8 per-channel with the
    same float semantics (what TFLite's converter emits for int8): activations
    shift by -128 (same scale), conv/dw filters re-quantised symmetric per
    output channel, biases re-scaled to in_scale*w_scale[c]."""
    from .tflite_reader_py import read  # local, dependency-free reader
    m = read(model_bytes)
    mb = ModelBuilder("int8 conversion of %s" % m["description"])
    tmap = {}
    new_w = {}
    # per-op filter / bias conversion
    for op in m["ops"]:
        if op["builtin"] in (OPC["CONV_2D"], OPC["DEPTHWISE_CONV_2D"]):
            x, w, b = op["inputs"][:3]
            tw, tb, tx = m["tensors"][w], m["tensors"][b], m["tensors"][x]
            wf = (tw["data"].astype(np.float32) - tw["zero_point"][0]) * tw["scale"][0]
            qdim = 0 if op["builtin"] == OPC["CONV_2D"] else 3
            axes = tuple(i for i in range(4) if i != qdim)
            amax = np.max(np.abs(wf), axis=axes)
            sc = np.where(amax > 0, amax / 127.0, 1.0).astype(np.float32)
            shp = [1, 1, 1, 1]
            shp[qdim] = -1
            wq = np.clip(np.round(wf / sc.reshape(shp)), -127, 127).astype(np.int8)
            bf = tb["data"].astype(np.float64) * tb["scale"][0]
            bsc = (np.float32(tx["scale"][0]) * sc).astype(np.float32)
            bq = np.round(bf / bsc.astype(np.float64)).astype(np.int32)
            new_w[w] = (wq, sc, qdim)
            new_w[b] = (bq, bsc, 0)
    for i, t in enumerate(m["tensors"]):
        if i in new_w:
            data, sc, qd = new_w[i]
            tmap[i] = mb.tensor(t["name"], t["shape"], data.dtype, scale=sc, zero_point=[0] * len(sc),
                                qdim=qd, data=data)
        elif t["type"] == T_UINT8:
            zp = [z - 128 for z in t["zero_point"]] if t["zero_point"] is not None else None
            data = None if t["data"] is None else (t["data"].astype(np.int16) - 128).astype(np.int8)
            tmap[i] = mb.tensor(t["name"], t["shape"], np.int8, scale=t["scale"], zero_point=zp, data=data)
        else:
            dt = {T_INT32: np.int32, T_FLOAT32: np.float32, T_INT8: np.int8}[t["type"]]
            tmap[i] = mb.tensor(t["name"], t["shape"], dt, scale=t["scale"], zero_point=t["zero_point"],
                                data=t["data"])
    for op in m["ops"]:
        mb.op(op["builtin"], [tmap[i] if i >= 0 else -1 for i in op["inputs"]], [tmap[i] for i in op["outputs"]],
              op["options_type"], op["options"])
    mb.inputs = [tmap[i] for i in m["inputs"]]
    mb.outputs = [tmap[i] for i in m["outputs"]]
    return mb.build()
