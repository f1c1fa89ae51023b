"""Fixtures of TANH and EMBEDDING_LOOKUP: numpy references that extend
tests.graph_reference's table (run_reference(buf, inputs, table=REF_TABLE)),
one-op models, the refused models and the text models that hold the two ops.

References, none from the product:
  8-bit TANH   the 256-entry table restated in numpy (dequantise in float32,
               libm's tanhf through ctypes, round(y * (1 / s_out)), + z_out,
               clamp), so the reference and quant.cc round the same function;
  float32 TANH float64 tanh, held to gamma(k) |y| + 2^-126 (tanh_f32_bound);
  EMBEDDING_LOOKUP  np.take(table, ids, 0) with GATHER's rule for an id
               outside the table (a zero row; tests.gather_models.gather_ref)."""
import ctypes
import ctypes.util

import numpy as np

from band_amd.tflite_synth import FGraph, ModelBuilder, QGraph, text_encoder
from tests import gather_models as G
from tests.fixed_point import round_half_away
from tests.graph_reference import TABLE

TANH, EMBEDDING_LOOKUP = 28, 7
F = np.float32

_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.tanhf.restype = ctypes.c_float
_libm.tanhf.argtypes = [ctypes.c_float]


def np_tanh_table(signed, s_in, z_in, s_out, z_out):
    """indexed by the input byte, as bh_lut_u8 reads it"""
    lo, hi = (-128, 127) if signed else (0, 255)
    inv = F(1.0) / F(s_out)
    table = np.zeros(256, np.uint8)
    for q in range(lo, hi + 1):
        x = F(F(s_in) * F(q - z_in))
        y = F(_libm.tanhf(float(x)))
        r = int(round_half_away(np.asarray(F(y * inv), np.float64))) + z_out
        table[q & 0xff] = np.uint8(min(max(r, lo), hi) & 0xff)
    return table


# (signed, s_in, z_in, s_out, z_out): a pooler's (the projection at 0.05, the output at 1 / 128 around the middle),
# a wide input that saturates both ends, a narrow one that stays in the linear part
TANH_Q = [(True, 0.05, 3, 1.0 / 128, 0), (False, 0.05, 131, 1.0 / 128, 128),
          (True, 0.25, -20, 1.0 / 128, 0), (False, 0.25, 108, 1.0 / 128, 128),
          (True, 0.004, 7, 1.0 / 256, -5), (False, 0.004, 135, 1.0 / 256, 123)]

# ulps of the library's tanhf: the device library's 16 as tests.float_harness takes them for GELU's tanh form; for
# glibc 2, the bound its own test tables (libm-test-ulps, x86_64) state for tanhf, not float_harness's 1, which GELU's
# bound can afford and a bare tanhf cannot (glibc's tanhf is 1.85 ulp off at x = -0.2813846).  The library's ulp count
# covers the rounding of its result; one ulp of a float32 y is at most 2^-23 |y| = 2 u |y|, so k = 2 ulps.
TANH_ULPS = {"host": 2, "device": 16}


def tanh_f32_bound(ref, where):
    """|float32 TANH - ref| allowed: gamma(k) |y| + 2^-126 with k = 2 TANH_ULPS[where] (host 4, device 32)"""
    k = 2 * TANH_ULPS[where]
    u = 2.0 ** -24
    return k * u / (1.0 - k * u) * np.abs(np.asarray(ref, np.float64)) + 2.0 ** -126


def tanh_f32_inputs():
    rng = np.random.default_rng(5)
    x = np.concatenate([rng.normal(0, 1.5, 4000), rng.uniform(-1e-3, 1e-3, 500), [0.0, -0.0, 9.0, -9.0, 20.0, -20.0, 88.0,
                        -88.0, 1e-30, -1e-30, 1e-40, 0.5493061, np.inf, -np.inf]])
    return x.astype(np.float32)


# ---- the reference table's entries ---------------------------------------------------------
def claims(om, o):
    return o.builtin in (TANH, EMBEDDING_LOOKUP)


def evaluate(om, o, vals):
    t_in, t_out = om.tensors[o.inputs[0]], om.tensors[o.outputs[0]]
    if o.builtin == EMBEDDING_LOOKUP:
        return [G.gather_ref(np.asarray(vals[o.inputs[1]]), vals[o.inputs[0]], 0)]
    x = vals[o.inputs[0]]
    if t_in.np_dtype == np.float32:
        return [np.tanh(x.astype(np.float64)).astype(np.float32)]
    signed = t_in.np_dtype == np.int8
    table = np_tanh_table(signed, float(t_in.scale[0]), int(t_in.zero_point[0]), float(t_out.scale[0]),
                          int(t_out.zero_point[0]))
    return [table[x.view(np.uint8)].view(t_in.np_dtype).reshape(t_out.shape)]


ENTRY = (claims, evaluate)
REF_TABLE = TABLE + G.ENTRIES + [ENTRY]


# ---- one-op models ---------------------------------------------------------------------------
def _q(dtype, scale, zp):
    return dict(scale=[scale], zero_point=[zp]) if scale is not None else {}


def raw_tanh(shape=(1, 4, 8), in_dtype=np.int8, out_dtype=None, in_q=(0.05, 3), out_q=(1.0 / 128, 0), out_shape=None):
    out_dtype = in_dtype if out_dtype is None else out_dtype
    mb = ModelBuilder("tanh")
    x = mb.tensor("x", list(shape), in_dtype, **(_q(in_dtype, *in_q) if in_q else {}))
    y = mb.tensor("y", list(out_shape or shape), out_dtype, **(_q(out_dtype, *out_q) if out_q else {}))
    mb.inputs.append(x)
    mb.op("TANH", [x], [y])
    mb.outputs.append(y)
    return mb.build()


def raw_lookup(table_shape, ids, dtype=np.int8, runtime_ids=True, index_dtype=np.int32, out_dtype=None, out_scale=None,
               const_table=True):
    """EMBEDDING_LOOKUP(ids, table): the table a constant filled by gather_models.fill (or an input), the ids an input
    (or a constant)"""
    ids = np.asarray(ids, index_dtype)
    out_dtype = dtype if out_dtype is None else out_dtype
    q8 = np.dtype(dtype).itemsize == 1
    mb = ModelBuilder("embedding_lookup")
    tq = _q(dtype, 0.05, 3) if q8 else {}
    n = int(np.prod(table_shape))
    values = (np.arange(n) + 1).astype(dtype).reshape(table_shape) if np.dtype(dtype).itemsize == 2 else G.fill(table_shape, dtype)
    tab = mb.tensor("table", list(table_shape), dtype, data=values if const_table else None, **tq)
    it = mb.tensor("ids", list(ids.shape), index_dtype, data=None if runtime_ids else ids)
    oq = _q(out_dtype, out_scale if out_scale is not None else 0.05, 3) if np.dtype(out_dtype).itemsize == 1 else {}
    y = mb.tensor("y", list(ids.shape) + list(table_shape[1:]), out_dtype, **oq)
    if not const_table:
        mb.inputs.append(tab)
    if runtime_ids:
        mb.inputs.append(it)
    mb.op("EMBEDDING_LOOKUP", [it, tab], [y])
    mb.outputs.append(y)
    return mb.build()


# id: (model, reason)
REFUSALS = {
    "tanh_int16": (lambda: raw_tanh(in_dtype=np.int16, in_q=(0.05, 0), out_q=(1.0 / 128, 0)),
                   "TANH: int8, uint8 and float32 only"),
    "tanh_types_differ": (lambda: raw_tanh(in_dtype=np.int8, out_dtype=np.uint8, out_q=(1.0 / 128, 128)),
                          "TANH output type differs from the input's"),
    "tanh_sizes_differ": (lambda: raw_tanh(out_shape=(1, 4, 4)), "TANH output size differs from the input's"),
    "tanh_no_quantisation": (lambda: raw_tanh(out_q=None), "TANH: missing quantization"),
    "lookup_dequantising": (lambda: raw_lookup((9, 16), [1, 2], np.int8, out_dtype=np.float32),
                            "EMBEDDING_LOOKUP table type differs from the output's"),
    "lookup_requantising": (lambda: raw_lookup((9, 16), [1, 2], np.int8, out_scale=0.25), "GATHER never requantises"),
    "lookup_constant_id_too_large": (lambda: raw_lookup((9, 16), [1, 9], runtime_ids=False),
                                     "GATHER constant index outside [0, axis_size)"),
    "lookup_float16_table": (lambda: raw_lookup((9, 16), [1, 2], np.float16), "GATHER params must be int8"),
}


# ---- models ------------------------------------------------------------------------------------
SMALL = dict(tokens=17, dim=48, heads=3, hidden=96, blocks=1, vocab=128, pooler=True, embedding_lookup=True)
TEXT_MODELS = {
    "text_pooler_i8": lambda **kw: text_encoder(np.int8, **dict(dict(SMALL, batch=2), **kw)),
    "text_pooler_f32": lambda **kw: text_encoder(np.float32, **dict(SMALL, **kw)),
    "text_pooler_hybrid": lambda **kw: text_encoder(np.float32, hybrid="symmetric", **dict(SMALL, **kw)),
}


def token_ids(buf, seed=0):
    from oracle.tflite_fb import Model as OModel
    om = OModel(buf)
    t = om.tensors[om.inputs[0]]
    look = next(o for o in om.operators if o.builtin == EMBEDDING_LOOKUP)
    vocab = om.tensors[look.inputs[1]].shape[0]
    return np.random.default_rng(seed).integers(0, vocab, t.shape).astype(t.np_dtype)


def token_ids_any(buf, seed=0):
    """token ids below the vocabulary size for a text model that reads its table by GATHER or EMBEDDING_LOOKUP"""
    from oracle.tflite_fb import Model as OModel
    om = OModel(buf)
    t = om.tensors[om.inputs[0]]
    op = next(o for o in om.operators if o.builtin in (EMBEDDING_LOOKUP, G.GATHER))
    vocab = om.tensors[op.inputs[1 if op.builtin == EMBEDDING_LOOKUP else 0]].shape[0]
    return np.random.default_rng(seed).integers(0, vocab, t.shape).astype(t.np_dtype)
