"""Models for tests/test_lower_args_cpu.py and tests/test_lower_args_native.py:
small (8 x 8 or less) graphs of the conv / FC / pool / eltwise families, and
malformed variants of them that the Args functions (backend/hip/lower_args.h)
must refuse.  Each malformed model is a well-formed QGraph / FGraph model with
one field of one tensor or option table overwritten before it is serialised.

Run as a program (`python -m tests.lower_args_models NAME`) it prepares the
named malformed model on a kCPU executor and prints one JSON line: the
unsupported_ops of both workers, whether PrepareSubgraph was OK and its
message.  The tests run it as a child, so a crash of the lowering ends the
child and not pytest."""
import json
import sys

import numpy as np

from band_amd.tflite_synth import FGraph, QGraph, conv_options, pool_options


def _conv16(dtype=np.int8):
    g = QGraph(dtype, seed=11, name="conv16")
    x = g.input([1, 8, 8, 4], scale=0.05)
    y = g.conv(x, 16, k=3, act="NONE")
    g.output(y)
    return g, y


def pool_stride0():
    g = QGraph(np.int8, seed=1, name="pool_stride0")
    g.output(g.avgpool(g.input([1, 8, 8, 4]), (2, 2)))
    g.mb.ops[-1]["options"] = pool_options("VALID", 0, (2, 2))
    return g.mb.build()


def pool_output_shape():
    """options give 7 x 7, the tensor says 2 x 2"""
    g = QGraph(np.int8, seed=2, name="pool_output_shape")
    y = g.avgpool(g.input([1, 8, 8, 4]), (2, 2))
    g.output(y)
    g.mb.tensors[y]["shape"] = [1, 2, 2, 4]
    return g.mb.build()


def pool_filter0():
    g = QGraph(np.int8, seed=3, name="pool_filter0")
    g.output(g.avgpool(g.input([1, 8, 8, 4]), (2, 2), padding="SAME"))
    g.mb.ops[-1]["options"] = pool_options("SAME", 1, (0, 0))
    return g.mb.build()


def fc_output_shape():
    """8 units, the output tensor says [1, 2]"""
    g = QGraph(np.int8, seed=4, name="fc_output_shape")
    y = g.fully_connected(g.input([1, 16]), 8)
    g.output(y)
    g.mb.tensors[y]["shape"] = [1, 2]
    return g.mb.build()


def fc_depth0():
    g = QGraph(np.int8, seed=5, name="fc_depth0")
    g.output(g.fully_connected(g.input([1, 16]), 8))
    g.mb.tensors[g.mb.ops[-1]["inputs"][1]]["shape"] = [8, 0]
    return g.mb.build()


def conv_bias_count():
    """16 output channels, a bias of 4 entries"""
    g, _ = _conv16()
    bias = g.mb.tensors[g.mb.ops[-1]["inputs"][2]]
    bias["shape"] = [4]
    bias["scale"], bias["zero_point"] = bias["scale"][:4], [0] * 4
    g.mb.buffers[bias["buffer"]] = g.mb.buffers[bias["buffer"]][:16]
    return g.mb.build()


def conv_filter_scale_count():
    """16 output channels, 3 filter scales"""
    g, _ = _conv16()
    w = g.mb.tensors[g.mb.ops[-1]["inputs"][1]]
    w["scale"], w["zero_point"] = w["scale"][:3], [0] * 3
    return g.mb.build()


def conv_dilation0():
    g, _ = _conv16()
    g.mb.ops[-1]["options"] = conv_options("SAME", 1, "NONE", 0)
    return g.mb.build()


def float_conv_output_shape():
    g = FGraph(seed=6, name="float_conv_output_shape")
    y = g.conv(g.input([1, 8, 8, 4]), 8, k=3)
    g.output(y)
    g.mb.tensors[y]["shape"] = [1, 4, 4, 8]
    return g.mb.build()


def transpose_conv_output_shape():
    """4 x 4 at stride 2 (SAME) is 8 x 8; the output tensor says 5 x 5"""
    g = QGraph(np.int8, seed=7, name="transpose_conv_output_shape")
    y = g.transpose_conv(g.input([1, 4, 4, 4], scale=0.05), 8)
    g.output(y)
    g.mb.tensors[y]["shape"] = [1, 5, 5, 8]
    return g.mb.build()


# name -> (builder, index of the refused op, what the refusal must say)
MALFORMED = {
    "pool_stride0": (pool_stride0, 0, "strides must be >= 1"),
    "pool_output_shape": (pool_output_shape, 0, "pool output shape mismatch"),
    "fc_output_shape": (fc_output_shape, 0, "FC output shape mismatch"),
    "conv_bias_count": (conv_bias_count, 0, "bias element count differs from the output channels"),
    "conv_filter_scale_count": (conv_filter_scale_count, 0, "filter scale count is neither 1 nor the output channels"),
    "conv_dilation0": (conv_dilation0, 0, "dilations must be >= 1"),
    "pool_filter0": (pool_filter0, 0, "pool filter must be >= 1"),
    "fc_depth0": (fc_depth0, 0, "FULLY_CONNECTED depth must be >= 1"),
    # the float graph's constants sit behind two DEQUANTIZE ops
    "float_conv_output_shape": (float_conv_output_shape, 2, "conv output shape mismatch"),
    "transpose_conv_output_shape": (transpose_conv_output_shape, 0, "TRANSPOSE_CONV shape mismatch"),
}


def families():
    """One int8 graph through every family: conv 3x3 stride 2, grouped conv,
    depthwise 3x3 and 5x5, both pools, an ADD that folds into its conv and one
    that cannot (its conv operand has a second reader), TRANSPOSE_CONV and FC"""
    g = QGraph(np.int8, seed=21, name="families")
    x = g.input([1, 8, 8, 8], scale=0.05)
    a = g.conv(x, 16, k=3, stride=2, act="RELU6")           # 4 x 4 x 16
    b = g.conv(a, 16, k=3, act="NONE", groups=2)
    c = g.dwconv(b, k=3, act="RELU6")
    d = g.dwconv(c, k=5, act="NONE")
    e = g.add(g.conv(d, 16, k=1, act="NONE"), c)            # folds into the 1x1 conv
    f = g.conv(e, 16, k=1, act="NONE")
    h = g.add(f, e)                                         # f is read again below: stays an ADD
    m = g.maxpool(f, (2, 2), 1, padding="SAME")
    u = g.transpose_conv(g.add(h, m), 8, k=3, stride=2)     # 8 x 8 x 8
    p = g.avgpool(u, (2, 2), stride=2)                      # 4 x 4 x 8
    g.output(g.fully_connected(g.reshape(p, [1, 128]), 10))
    return g.build()


def float_families():
    """the float32 forms: conv, depthwise, pools, ADD, FC"""
    g = FGraph(seed=22, name="float_families")
    x = g.input([1, 8, 8, 4])
    a = g.conv(x, 8, k=3, stride=2)
    b = g.dwconv(a, k=3)
    c = g.add(g.maxpool(b, (2, 2), 1), a)
    p = g.avgpool(c, (2, 2), stride=2)
    g.output(g.fully_connected(g.reshape(p, [1, 32]), 5))
    return g.build()


def _child(name):
    from band_amd import DeviceFlag, HipModel, HipModelExecutor
    m = HipModel(0)
    assert m.FromBuffer(MALFORMED[name][0]()).ok()
    spec = HipModelExecutor(0, 0, DeviceFlag.kCPU).InvestigateModelSpec(m)
    st = HipModelExecutor(0, 0, DeviceFlag.kCPU).PrepareSubgraph(m)
    print(json.dumps({"cpu": sorted(spec.unsupported_ops[DeviceFlag.kCPU]),
                      "gpu": sorted(spec.unsupported_ops[DeviceFlag.kGPU]), "ok": bool(st.ok()),
                      "message": st.message()}))


if __name__ == "__main__":
    _child(sys.argv[1])
