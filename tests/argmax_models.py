"""ARG_MAX / ARG_MIN test fixtures: the reference helper and the models.

The oracle does not know these ops, so the expected output of a model is the
oracle's run of its twin WITHOUT the ARG_MAX / ARG_MIN tails (same seed, same
weights: arg_max draws nothing from the generator) followed by arg_ref, the
restated loop of TFLite's reference_ops::ArgMinMax: start at element 0,
replace only on a strict comparison.  The first extreme wins; a float NaN is
never greater (or smaller), so it is selected only as element 0."""
import numpy as np

from band_amd.tflite_synth import OPT, QGraph, Table, deeplab_v3_mobilenet_v2
from oracle.tflite_fb import Model as OModel
from tests.graph_reference import run_reference


def arg_ref(x, axis=-1, minimum=False, out=np.int32):
    """first-extreme index of x along axis, the axis removed"""
    x = np.asarray(x)
    if x.dtype.kind in "iu":
        # np.argmax / np.argmin return the first occurrence and compare in the array's own type
        return (np.argmin if minimum else np.argmax)(x, axis=axis).astype(out)
    v = np.moveaxis(x, axis, -1)
    flat = v.reshape(-1, v.shape[-1])
    res = np.zeros(flat.shape[0], out)
    for r, row in enumerate(flat):  # floats: the sequential loop itself (np.argmax treats NaN as the maximum)
        best, idx = row[0], 0
        for i in range(1, len(row)):
            if (row[i] < best) if minimum else (row[i] > best):
                best, idx = row[i], i
        res[r] = idx
    return res.reshape(v.shape[:-1])


def tied_pixels(logits):
    """pixels of [.., C] logits whose maximum is tied with first index != last index"""
    m = logits.max(axis=-1, keepdims=True)
    first = np.argmax(logits == m, axis=-1)
    last = logits.shape[-1] - 1 - np.argmax((logits == m)[..., ::-1], axis=-1)
    return int((first != last).sum())


def _zoo(tails, seed=23):
    g = QGraph(np.int8, seed=seed, name="argmax_zoo")
    x = g.input([1, 6, 5, 8], scale=0.05)
    a = g.conv(x, 16, k=3, act="NONE")
    # a 4-D uint8 tensor (QUANTIZE int8 -> uint8) for the ARG_MIN over axis 1
    _, s_a, z_a = g.meta[a]
    u = g.mb.tensor(g._name("u8"), [1, 6, 5, 16], np.uint8, scale=[s_a], zero_point=[z_a + 128])
    g.meta[u] = ([1, 6, 5, 16], s_a, z_a + 128)
    g.mb.op("QUANTIZE", [a], [u], OPT["QuantizeOptions"], Table())
    sm = g.softmax(g.fully_connected(g.reshape(a, [1, 6 * 5 * 16]), 37))
    f = g.dequantize(a)
    b = g.conv(x, 21, k=1, act="NONE")
    if not tails:
        for t in (sm, u, f, b):
            g.output(t)
        return g.build()
    g.output(g.arg_max(sm, axis=-1, output=np.int64))
    g.output(g.arg_max(u, axis=1, output=np.int32, minimum=True, axis_dtype=np.int64))
    g.output(g.arg_max(f, axis=3, output=np.int32))
    g.output(b)  # the next ARG_MAX's input is a model output too
    g.output(g.arg_max(b, axis=3, output=np.int64))
    return g.build()


def argmax_zoo():
    """FC -> SOFTMAX -> ARG_MAX (axis -1, int64); ARG_MIN over axis 1 of a 4-D
    uint8 tensor with an int64 axis tensor; a float32 ARG_MAX behind a
    DEQUANTIZE; an ARG_MAX whose input is also a model output"""
    return _zoo(True)


def argmax_zoo_twin():
    return _zoo(False)


def argmax_zoo_ref(x):
    """expected outputs of argmax_zoo for input x, from the twin's [softmax, uint8, float, logits]"""
    twin = argmax_zoo_twin()
    vals = run_reference(twin, x)
    sm, u, f, b = [vals[t] for t in OModel(twin).outputs]
    return [arg_ref(sm, -1, out=np.int64), arg_ref(u, 1, minimum=True), arg_ref(f, 3), b, arg_ref(b, 3, out=np.int64)]


def deeplab_logits(size, x):
    """the reference's [1, size, size, 21] logits of the DeepLab twin (argmax=None)"""
    buf = deeplab_v3_mobilenet_v2(np.int8, size=size)
    return run_reference(buf, x)[OModel(buf).outputs[0]]
