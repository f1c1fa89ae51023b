"""Float lowering (LowerFloat: OHWI -> [K][out_c] transposition, fp16
DEQUANTIZE folding, FloatActRange, padding) and the kCPU worker's float
kernels (CpuConvF32 ... CpuSoftmaxF32), op by op: small float graphs run with
every op output viewed, each op compared with its float64 reference evaluated
on the executor's own input tensors of that op, at the per-op bound of
tests/float_harness.py, so nothing accumulates across layers.  The same cases
run on the GPU worker in tests/test_float_kernels_gpu.py."""
import numpy as np
import pytest

from band_amd import DeviceFlag
from tests import float_harness as H
from tests.glue_models import float_edge_zoo, float_zoo
from tests.test_float_cpu import assert_float_close

GRAPHS = {"float_zoo": float_zoo, "float_edge_zoo": float_edge_zoo}


def graph_feed(om, seed=5):
    """uniform(-1, 1) + 0.5: the offset keeps a padding mistake from cancelling"""
    rng = np.random.default_rng(seed)
    return {t: (rng.uniform(-1, 1, om.tensors[t].shape) + 0.5).astype(np.float32) for t in om.inputs}


def nonfinite_feed(om):
    """+inf, -inf and NaN at three known positions of each image"""
    feed = graph_feed(om, seed=6)
    for x in feed.values():
        flat = x.reshape(x.shape[0], -1)
        flat[:, 7], flat[:, flat.shape[1] // 2], flat[:, -3] = np.inf, -np.inf, np.nan
    return feed


def check_all_ops(buf, flag, worker, feed_fn, what):
    from oracle.tflite_fb import Model as OModel
    om, (vals,) = H.run_executor(buf, [feed_fn(OModel(buf))], flag, worker, view_all=True)
    return H.check_graph_ops(om, vals, what)[0]


def check_outputs_only(buf, flag, worker, what):
    """only the outputs viewed: the DEQUANTIZE folding is active; three runs
    of one executor (on the GPU worker the third replays the captured graph)"""
    from oracle.tflite_fb import Model as OModel
    feeds = [graph_feed(OModel(buf), seed) for seed in (5, 8, 9)]
    om, runs = H.run_executor(buf, feeds, flag, worker, view_all=False)
    for it, (feed, vals) in enumerate(zip(feeds, runs)):
        ref = H.graph_reference(om, feed)
        for t in om.outputs:
            assert_float_close(vals[t], ref[t], "%s run %d tensor %d" % (what, it, t))


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_every_op_cpu_worker(name):
    worst = check_all_ops(GRAPHS[name](), DeviceFlag.kCPU, 0, graph_feed, name + " kCPU")
    assert worst and max(worst.values()) <= 1.0


@pytest.mark.parametrize("name", sorted(GRAPHS))
def test_outputs_only_cpu_worker(name):
    check_outputs_only(GRAPHS[name](), DeviceFlag.kCPU, 0, name + " kCPU")


def test_float_edge_zoo_covers_its_edges():
    """the graph holds what its docstring says (a later edit cannot drop an edge silently)"""
    from oracle.tflite_fb import Model as OModel
    om = OModel(float_edge_zoo())
    T, ops = om.tensors, om.operators
    assert T[om.inputs[0]].shape[0] == 2
    consts = {t.np_dtype for t in T if t.is_const and t.np_dtype in (np.float16, np.float32)}
    assert consts == {np.float16, np.float32}
    conv = [o for o in ops if o.name == "CONV_2D"]
    assert any(len(o.inputs) == 2 for o in conv)
    assert any(T[o.inputs[1]].shape[1:] == [1, 1, 129] for o in conv)
    assert any(o.name == "FULLY_CONNECTED" and o.inputs[2] == -1 for o in ops)
    assert any(o.name == "DEPTHWISE_CONV_2D" and o.options.scalar(3, "i", 1) == 3 for o in ops)
    assert any(o.options.scalar(1, "i", 1) == 2 and T[o.inputs[0]].shape[1] % 2 == 0 for o in conv)
    assert any(o.name == "AVERAGE_POOL_2D" and o.options.scalar(0, "b", 0) == 0 for o in ops)
    assert any(o.name == "MUL" and T[o.inputs[0]].shape != T[o.outputs[0]].shape for o in ops)
    assert {41, 99, 76} <= {o.builtin for o in ops}  # SUB, SQUARED_DIFFERENCE, RSQRT


def test_conv_f32_split_is_host_only():
    """bh_conv2d_f32_split answers without a device, and the GPU cases of
    tests/test_float_kernels_gpu.py take every split-K factor"""
    import ctypes

    from band_amd import _abi
    from tests.test_float_kernels_gpu import CONV_CASES, conv_case, conv_params
    lib = _abi.load()
    taken = set()
    for name in CONV_CASES:
        x, w, _, g, ks = conv_case(name)
        p = conv_params(x, w, g, "NONE")
        assert lib.bh_conv2d_f32_split(ctypes.byref(p)) == ks, name
        taken.add(ks)
    assert taken == {1, 2, 4, 8, 16}


def test_nonfinite_cpu_worker():
    """NaN and +-inf come out of the kCPU worker exactly where the float64
    model of TFLite's std::min(std::max(v, lo), hi) puts them (the model the
    GPU kernels are held to in tests/test_float_kernels_gpu.py)"""
    worst = check_all_ops(float_zoo(), DeviceFlag.kCPU, 0, nonfinite_feed, "float_zoo kCPU non-finite")
    assert worst
