"""Fixtures of CAST and of the padded text models: the conversion rule restated
in Python integers, the sources with their edge values, the refused models and
text_encoder(mask=True) with its inputs.

Reference: for values inside the target's range numpy's astype; outside it this
backend's own rule: float32 -> integer truncates toward
zero, NaN gives 0, a value outside the range saturates; integer -> integer
keeps the low bits; integer -> float32 rounds to nearest.  cast_ref states the
float32 -> integer part with Python's exact integers, nothing of the product."""
import math

import numpy as np

from band_amd.tflite_synth import ModelBuilder, OPT, Table, text_encoder
from tests import gather_models as G
from tests import tanh_lookup_models as T

CAST = 53
TYPES = (np.uint8, np.int32, np.int64, np.float32)
CODE = {np.dtype(np.uint8): 1, np.dtype(np.int32): 2, np.dtype(np.int64): 3, np.dtype(np.float32): 4}
COUNTS = (1, 63, 64, 65, 4099)


def cast_ref(x, dtype):
    x, dtype = np.asarray(x), np.dtype(dtype)
    if x.dtype != np.float32 or dtype == np.float32:
        return x.astype(dtype)  # integer sources, and float32 -> float32: defined for every value
    info = np.iinfo(dtype)
    out = np.zeros(x.shape, dtype)
    flat = out.reshape(-1)
    for i, v in enumerate(x.reshape(-1).tolist()):
        if math.isnan(v):
            r = 0
        elif math.isinf(v):
            r = info.max if v > 0 else info.min
        else:
            r = min(max(math.trunc(v), info.min), info.max)
        flat[i] = r
    return out


def source(dtype, count, seed=0):
    """`count` values of dtype: the edge values first (as many as fit), then seeded ones over the whole range"""
    dtype = np.dtype(dtype)
    rng = np.random.default_rng(seed + count)
    if dtype == np.float32:
        edge = [np.nan, np.inf, -np.inf, 2.0 ** 31, -2.0 ** 31, 2.0 ** 63, -2.0 ** 63, -0.5, 0.5, -0.0, 255.9, 256.0, -1.0,
                -0.99, 2147483520.0, -2147483904.0, 1e10, -1e10, 3e38, -3e38, 9.2233715e18, 1e-40, 16777217.0, 254.5]
        rest = np.concatenate([rng.normal(0, 300, count), rng.normal(0, 3e9, count), rng.normal(0, 1e19, count)])
        rng.shuffle(rest)
    else:
        info = np.iinfo(dtype)
        edge = [v for v in (0, 1, -1, 255, 256, -128, 2 ** 24 + 1, -(2 ** 24) - 1, 2 ** 31 - 1, -(2 ** 31), 2 ** 31, 2 ** 32 + 5,
                            2 ** 53 + 1, info.max, info.min) if info.min <= v <= info.max]
        rest = rng.integers(info.min, info.max, count, dtype=dtype, endpoint=True)
    vals = np.concatenate([np.asarray(edge, dtype), np.asarray(rest, dtype)])
    return vals[:count] if count >= len(edge) else np.asarray(edge, dtype)[(np.arange(count) * 7) % len(edge)]


def raw_cast(shape, in_dtype, out_dtype, in_q=None, out_q=None):
    mb = ModelBuilder("cast")
    x = mb.tensor("x", list(shape), in_dtype, **(dict(scale=[in_q[0]], zero_point=[in_q[1]]) if in_q else {}))
    y = mb.tensor("y", list(shape), out_dtype, **(dict(scale=[out_q[0]], zero_point=[out_q[1]]) if out_q else {}))
    mb.inputs.append(x)
    mb.op("CAST", [x], [y], OPT["CastOptions"], Table())
    mb.outputs.append(y)
    return mb.build()


REFUSALS = {
    "cast_quantised_input": (lambda: raw_cast((1, 8), np.uint8, np.float32, in_q=(0.05, 3)), "QUANTIZE / DEQUANTIZE"),
    "cast_quantised_output": (lambda: raw_cast((1, 8), np.float32, np.uint8, out_q=(0.05, 3)), "QUANTIZE / DEQUANTIZE"),
    "cast_int8": (lambda: raw_cast((1, 8), np.int8, np.float32), "CAST types must be uint8, int32, int64 or float32"),
    "cast_float16": (lambda: raw_cast((1, 8), np.float32, np.float16), "CAST types must be uint8, int32, int64 or float32"),
}


# ---- the reference table's entry -------------------------------------------------------------
def claims(om, o):
    return o.builtin == CAST


def evaluate(om, o, vals):
    return [cast_ref(vals[o.inputs[0]], om.tensors[o.outputs[0]].np_dtype).reshape(om.tensors[o.outputs[0]].shape)]


REF_TABLE = T.REF_TABLE + [(claims, evaluate)]

# ---- the padded text models ----------------------------------------------------------------------
SMALL = dict(tokens=17, dim=48, heads=3, hidden=96, vocab=128, blocks=2, mask=True, pooler=True, embedding_lookup=True)
PADDED = {
    "padded_text_i8": lambda **kw: text_encoder(np.int8, **dict(dict(SMALL, batch=2), **kw)),
    "padded_text_f32": lambda **kw: text_encoder(np.float32, **dict(dict(SMALL, batch=2), **kw)),
    "padded_text_hybrid": lambda **kw: text_encoder(np.float32, hybrid="symmetric", **dict(dict(SMALL, batch=2), **kw)),
}
MASKED_TOKENS = (5, 0)  # trailing tokens masked in the batch items (item b: MASKED_TOKENS[(b + seed) % 2])


def inputs(buf, seed=0):
    """{ids tensor: ids, mask tensor: 1 / 0}"""
    from oracle.tflite_fb import Model as OModel
    om = OModel(buf)
    t_ids, t_mask = om.inputs
    ids = T.token_ids_any(buf, seed)
    mask = np.ones(om.tensors[t_mask].shape, np.int32)
    for b in range(mask.shape[0]):
        n = MASKED_TOKENS[(b + seed) % 2]
        if n:
            mask[b, -n:] = 0
    return {t_ids: ids, t_mask: mask}
