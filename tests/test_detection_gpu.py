"""TFLite_Detection_PostProcess on the MI355X (kernels/detection.hip behind
BAND_HIP_GPU_DETECTION=1): the launcher, the executor plumbing (support
report, whole-model subgraphs, the folded 8-bit DEQUANTIZE front, job
batching), and an engine with GPU workers only - every output exact
(assert_array_equal) against oracle.detection_postprocess / OracleInterpreter.

The knob is latched per executor at construction: monkeypatch.setenv before
the constructor is the switch, and the knob-off checks sit next to the
knob-on ones.
"""
import ctypes
import functools

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, tflite_synth as S
from band_amd.engine import Engine, JobStatus, Model, SchedulerType, make_config, kBandOk
from oracle.detection_postprocess import detection_postprocess, read_flexbuffer_map
from oracle.runner import OracleInterpreter
from oracle.tflite_fb import Model as OModel
from tests.glue_models import split_zoo
from tests.test_detection_cpu import _postprocess_only

pytestmark = pytest.mark.gpu

KNOB = "BAND_HIP_GPU_DETECTION"
OPTS = dict(max_detections=10, max_classes_per_detection=1, use_regular_nms=False, nms_score_threshold=0.3,
            nms_iou_threshold=0.5, num_classes=3, y_scale=10.0, x_scale=10.0, h_scale=5.0, w_scale=5.0)


class _Launcher:
    """bh_detection_postprocess over float inputs; scratch and output buffers
    are allocated once (for `batch` images) and reused by every run()"""

    def __init__(self, lib, anchors, opts, classes_with_background, batch=1):
        from band_amd import _abi
        from band_amd.device import DeviceBuffer
        self.lib, self._abi, self._buf = lib, _abi, DeviceBuffer
        self.n, self.cwb, self.batch = anchors.shape[0], classes_with_background, batch
        self.d = int(opts["max_detections"])
        self.anchors = DeviceBuffer.from_array(np.ascontiguousarray(anchors, np.float32))
        self.scratch = DeviceBuffer(lib.bh_detection_scratch_bytes(batch, self.n))
        # poisoned: a kernel that read scratch it had not written would show
        self.scratch.upload(np.full(self.scratch.nbytes, 0xff, np.uint8))
        self.outs = [DeviceBuffer(4 * batch * k) for k in (self.d * 4, self.d, self.d, 1)]
        for o in self.outs:
            o.upload(np.full(o.nbytes, 0x7f, np.uint8))
        self.p = _abi.DetectionParams(
            batch=batch, num_boxes=self.n, num_classes=int(opts["num_classes"]),
            num_classes_with_background=classes_with_background, max_detections=self.d,
            score_threshold=opts["nms_score_threshold"], iou_threshold=opts["nms_iou_threshold"],
            scale_y=opts["y_scale"], scale_x=opts["x_scale"], scale_h=opts["h_scale"], scale_w=opts["w_scale"],
            anchors=self.anchors.value, out_boxes=self.outs[0].value, out_classes=self.outs[1].value,
            out_scores=self.outs[2].value, out_num=self.outs[3].value, scratch=self.scratch.value)

    def run(self, box_enc, scores):
        be = self._buf.from_array(np.ascontiguousarray(box_enc, np.float32))
        cs = self._buf.from_array(np.ascontiguousarray(scores, np.float32))
        self.p.box_encodings, self.p.class_scores = be.value, cs.value
        self._abi.check(self.lib.bh_detection_postprocess(ctypes.byref(self.p), None), "bh_detection_postprocess")
        b, d = self.batch, self.d
        return [o.download(np.float32, s) for o, s in zip(self.outs, ((b, d, 4), (b, d), (b, d), (b,)))]


def _check(got, box_enc, scores, anchors, opts):
    """every image of a launch against its own oracle run"""
    for img in range(got[0].shape[0]):
        ref = detection_postprocess(box_enc[img], scores[img], anchors, opts)
        for k, name in enumerate(("boxes", "classes", "scores", "num")):
            np.testing.assert_array_equal(got[k][img].reshape(-1), ref[k].reshape(-1),
                                          err_msg="image %d %s" % (img, name))
    return ref


# (n, classes, background, seed, max_det, score_th) -> candidates (the
# reference's count): one box; N not a multiple of 64; every anchor a
# candidate over 17 distinct scores; none; more candidates than one sweep of
# the workgroup; a 91-wide row
LAUNCHER_CASES = [((1, 1, 0, 9, 3, 0.3), 1), ((50, 3, 1, 0, 10, 0.3), 49), ((70, 3, 1, 6, 7, 0.3), 68),
                  ((300, 7, 0, 1, 25, 0.5), 298), ((1000, 2, 1, 2, 100, 0.0), 1000), ((64, 5, 1, 3, 5, 1.1), 0),
                  ((6000, 4, 1, 4, 100, 0.0), 6000), ((2500, 90, 1, 7, 25, 0.6), 2500)]


@pytest.mark.parametrize("case,candidates", LAUNCHER_CASES)
def test_launcher_vs_oracle(gpu_lib, case, candidates):
    n, classes, background, seed, max_det, score_th = case
    buf, feeds = _postprocess_only(n, classes, background, seed, max_det, score_th)
    om = OModel(buf)
    op = om.operators[0]
    opts = read_flexbuffer_map(op.custom_options)
    be, cs, anchors = feeds[op.inputs[0]], feeds[op.inputs[1]], om.tensors[op.inputs[2]].data
    best = cs[0][:, background:].max(axis=1)
    assert int((best >= np.float32(score_th)).sum()) == candidates
    got = _Launcher(gpu_lib, anchors, opts, classes + background).run(be, cs)
    ref = _check(got, be, cs, anchors, opts)
    assert 0 <= int(ref[3][0]) <= min(candidates, max_det)
    if candidates == 0:
        assert got[3][0] == 0 and not any(g.any() for g in got)


def _grid_anchors(n, h=0.2, w=0.2):
    """n well-separated anchors (no two decoded boxes overlap)"""
    side = int(np.ceil(np.sqrt(n)))
    yx = np.array([((i // side + 0.5) / side, (i % side + 0.5) / side) for i in range(n)], np.float32)
    return np.concatenate([yx, np.full((n, 1), h / side, np.float32), np.full((n, 1), w / side, np.float32)], 1)


def test_launcher_signed_zero_scores_tie_by_index(gpu_lib):
    """+0.0 and -0.0 are one score (the reference's stable sort compares them
    equal): with threshold 0.0 the anchor index alone orders them"""
    n = 12
    anchors = _grid_anchors(n)
    opts = dict(OPTS, nms_score_threshold=0.0, num_classes=1, max_detections=n)
    cs = np.zeros((1, n, 1), np.float32)
    cs[0, ::2, 0] = -0.0
    cs[0, 5, 0] = -1.0  # below the threshold
    assert np.signbit(cs[0, 0, 0]) and not np.signbit(cs[0, 1, 0])
    be = np.zeros((1, n, 4), np.float32)
    got = _Launcher(gpu_lib, anchors, opts, 1).run(be, cs)
    _check(got, be, cs, anchors, opts)
    assert got[3][0] == n - 1
    # boxes come out in anchor order: decoded ycenter / xcenter of the anchors
    order = [i for i in range(n) if i != 5]
    np.testing.assert_allclose((got[0][0, :n - 1, 0] + got[0][0, :n - 1, 2]) / 2, anchors[order, 0], rtol=1e-6)


def test_launcher_nan_score_is_no_candidate(gpu_lib):
    n = 70
    rng = np.random.default_rng(5)
    anchors = _grid_anchors(n)
    opts = dict(OPTS, num_classes=1, max_detections=n)
    cs = rng.uniform(0.4, 0.9, (1, n, 1)).astype(np.float32)
    cs[0, [3, 64, 69], 0] = np.nan
    be = rng.normal(0, 0.1, (1, n, 4)).astype(np.float32)
    got = _Launcher(gpu_lib, anchors, opts, 1).run(be, cs)
    _check(got, be, cs, anchors, opts)
    assert got[3][0] == n - 3 and not np.isnan(got[2]).any()


def test_launcher_zero_area_boxes_never_suppress(gpu_lib):
    """anchors with h = 0 decode to area 0: the IoU takes the `area <= 0 ->
    0` branch, so identical degenerate boxes all survive"""
    n = 9
    anchors = np.tile(np.array([[0.5, 0.5, 0.0, 0.3]], np.float32), (n, 1))
    anchors[6:] = [0.5, 0.5, 0.3, 0.3]  # three identical proper boxes: one survives
    opts = dict(OPTS, num_classes=2, max_detections=n)
    rng = np.random.default_rng(8)
    cs = rng.uniform(0.5, 1.0, (1, n, 3)).astype(np.float32)
    be = np.zeros((1, n, 4), np.float32)
    got = _Launcher(gpu_lib, anchors, opts, 3).run(be, cs)
    _check(got, be, cs, anchors, opts)
    assert got[3][0] == 7


def test_launcher_fewer_candidates_than_max_detections(gpu_lib):
    n, max_det = 130, 40
    rng = np.random.default_rng(11)
    anchors = _grid_anchors(n)
    opts = dict(OPTS, max_detections=max_det)
    cs = rng.uniform(0.0, 0.25, (1, n, 4)).astype(np.float32)
    cs[0, [2, 66, 129], 2] = [0.5, 0.9, 0.7]
    be = rng.normal(0, 0.1, (1, n, 4)).astype(np.float32)
    got = _Launcher(gpu_lib, anchors, opts, 4).run(be, cs)
    _check(got, be, cs, anchors, opts)
    assert got[3][0] == 3
    assert not got[0][0, 3:].any() and not got[1][0, 3:].any() and not got[2][0, 3:].any()
    np.testing.assert_array_equal(got[1][0, :3], [1, 1, 1])  # class 2 of 4 with one background class


def test_launcher_batch_of_three_images(gpu_lib):
    n = 333
    buf, feeds = _postprocess_only(n, 5, 1, 21, 20, 0.4)
    om = OModel(buf)
    op = om.operators[0]
    opts = read_flexbuffer_map(op.custom_options)
    anchors = om.tensors[op.inputs[2]].data
    rng = np.random.default_rng(22)
    be = rng.normal(0, 1, (3, n, 4)).astype(np.float32)
    cs = (rng.integers(0, 17, (3, n, 6)) / 16.0).astype(np.float32)
    cs[1] *= 0.5  # fewer candidates in the middle image
    cs[2, :, :] = 0.0  # none in the last
    got = _Launcher(gpu_lib, anchors, opts, 6, batch=3).run(be, cs)
    _check(got, be, cs, anchors, opts)
    assert got[3][0] > 0 and got[3][2] == 0


def test_launcher_second_launch_with_fewer_candidates(gpu_lib):
    """the scratch of a launch with many candidates, reused by one with few
    and then by one with none: nothing stale is seen"""
    n = 1500
    buf, feeds = _postprocess_only(n, 3, 1, 30, 50, 0.0)
    om = OModel(buf)
    op = om.operators[0]
    opts = read_flexbuffer_map(op.custom_options)
    anchors = om.tensors[op.inputs[2]].data
    run = _Launcher(gpu_lib, anchors, opts, 4)
    be, cs = feeds[op.inputs[0]], feeds[op.inputs[1]]
    _check(run.run(be, cs), be, cs, anchors, opts)
    run.p.score_threshold = 0.99
    few = dict(opts, nms_score_threshold=0.99)
    assert 0 < int((cs[0][:, 1:].max(axis=1) >= np.float32(0.99)).sum()) < n
    _check(run.run(be, cs), be, cs, anchors, few)
    cs0 = np.zeros_like(cs)
    got = run.run(be, cs0)
    _check(got, be, cs0, anchors, few)
    assert got[3][0] == 0


def test_launcher_refuses_bad_geometry(gpu_lib):
    run = _Launcher(gpu_lib, _grid_anchors(8), OPTS, 4)
    run.run(np.zeros((1, 8, 4), np.float32), np.zeros((1, 8, 4), np.float32))
    good = {f: getattr(run.p, f) for f in ("num_boxes", "num_classes", "max_detections", "batch", "anchors",
                                           "out_num", "scratch", "class_scores")}
    for field, bad in (("num_boxes", 0), ("num_classes", 0), ("num_classes", 5), ("max_detections", 0),
                       ("batch", 0), ("anchors", None), ("out_num", None), ("scratch", None),
                       ("class_scores", None)):
        setattr(run.p, field, bad)
        assert gpu_lib.bh_detection_postprocess(ctypes.byref(run.p), None) != 0, field
        setattr(run.p, field, good[field])
    assert gpu_lib.bh_detection_postprocess(None, None) != 0
    assert gpu_lib.bh_detection_postprocess(ctypes.byref(run.p), None) == 0


# ---- executor level ---------------------------------------------------------

def _executor(buf, mid, monkeypatch, knob="1"):
    if knob is None:
        monkeypatch.delenv(KNOB, raising=False)
    else:
        monkeypatch.setenv(KNOB, knob)
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(mid, 1, DeviceFlag.kGPU)
    ex._model_ref = m
    return m, ex, SubgraphKey(mid, 1)


def _inputs(om, n, seed):
    t = om.tensors[om.inputs[0]]
    rng = np.random.default_rng(seed)
    lo, hi = (-128, 128) if t.np_dtype == np.int8 else (0, 256)
    return [rng.integers(lo, hi, t.shape).astype(t.np_dtype) for _ in range(n)]


def _run_and_compare(ex, key, om, x, ref, what=""):
    ex.GetTensorView(key, om.inputs[0]).GetData()[...] = x
    assert ex.ExecuteSubgraph(key).ok()
    for o in om.outputs:
        got = ex.GetTensorView(key, o).GetData()
        np.testing.assert_array_equal(got, ref[o].reshape(got.shape), err_msg="%s output %d" % (what, o))


@pytest.mark.parametrize("graph", [False, True])
def test_split_zoo_whole_on_gpu(gpu_lib, monkeypatch, graph):
    buf = split_zoo()
    om = OModel(buf)
    m, ex, key = _executor(buf, 41, monkeypatch)
    assert ex.InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kGPU] == set()
    ex.SetUseGraph(graph)
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    for seed in (0, 1, 2):  # with the graph on: captured on the second run, replayed on the third
        x = _inputs(om, 1, seed)[0]
        ref = OracleInterpreter(om).run({om.inputs[0]: x})
        assert int(ref[om.outputs[3]][0]) == 8
        _run_and_compare(ex, key, om, x, ref, "seed %d" % seed)
    # the knob off (unset, or 0) in the same process: today's placement
    for mid, knob in ((42, None), (43, "0")):
        m0, ex0, _ = _executor(buf, mid, monkeypatch, knob=knob)
        bad = ex0.InvestigateModelSpec(m0).unsupported_ops[DeviceFlag.kGPU]
        custom = {i for i, op in enumerate(om.operators) if op.builtin == 32}
        feeding = {i for i, op in enumerate(om.operators) if op.builtin == 6}
        assert len(custom) == 1 and len(feeding) == 2 and bad == custom | feeding
        st = ex0.PrepareSubgraph(m0)
        assert not st.ok() and "cannot run op" in st.message()
    # ... and the knob-on executor built before them still runs the op
    x = _inputs(om, 1, 3)[0]
    _run_and_compare(ex, key, om, x, OracleInterpreter(om).run({om.inputs[0]: x}), "after knob-off executors")


EDET_SIZE = 128


@functools.lru_cache(maxsize=None)
def _edet():
    buf = S.efficientdet_lite2(np.int8, size=EDET_SIZE)
    om = OModel(buf)
    xs = _inputs(om, 4, 77)
    refs = [OracleInterpreter(om).run({om.inputs[0]: x}) for x in xs]
    for r in refs:
        for a in r.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
    return buf, om, xs, refs


def _dequant_ops(om):
    custom = next(op for op in om.operators if op.builtin == 32)
    return custom, [i for i, op in enumerate(om.operators) if op.builtin == 6 and op.outputs[0] in custom.inputs]


def test_efficientdet_8bit_front(gpu_lib, monkeypatch):
    buf, om, xs, refs = _edet()
    assert om.tensors[om.operators[-1].inputs[2]].shape[0] == 3069
    assert int(refs[0][om.outputs[3]][0]) == 25
    m, ex, key = _executor(buf, 44, monkeypatch)
    assert ex.InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kGPU] == set()
    assert ex.PrepareSubgraph(m).ok()
    for i in (0, 1, 0):  # eager, capture, replay
        _run_and_compare(ex, key, om, xs[i], refs[i], "input %d" % i)
    custom, deq = _dequant_ops(om)
    assert len(deq) == 2
    rows = ex.ProfileSubgraph(key, iters=1)
    assert not [r for r in rows if r["op_index"] in deq], "a DEQUANTIZE launch feeds the op"
    det = [r for r in rows if r["kernel"] == "detection_postprocess_kernel"]
    assert len(det) == 1 and det[0]["op_index"] == om.operators.index(custom)
    # bytes read + written: the 8-bit scores and boxes, the anchors, the outputs
    n, d = 3069, 25
    assert det[0]["alg_bytes"] == n * 90 + n * 4 + n * 16 + 4 * (d * 4 + d + d + 1)
    # a view of the folded float tensor materialises it (and the op takes the float path)
    scores_f = custom.inputs[1]
    v = ex.GetTensorView(key, scores_f)
    _run_and_compare(ex, key, om, xs[2], refs[2], "materialised scores")
    np.testing.assert_array_equal(v.GetData(), refs[2][scores_f].reshape(v.GetData().shape))
    assert [r["op_index"] for r in ex.ProfileSubgraph(key, iters=1) if r["op_index"] in deq] == \
        [i for i in deq if om.operators[i].outputs[0] == scores_f]


def test_efficientdet_float_path_when_scores_are_an_output(gpu_lib, monkeypatch):
    """the dequantised class scores are also a model output: that DEQUANTIZE
    stays a launch and the op reads the float tensor (the boxes stay 8-bit)"""
    orig = S.QGraph.detection_postprocess

    def with_scores_out(self, boxes_f, scores_f, *a, **k):
        self.output(scores_f)
        return orig(self, boxes_f, scores_f, *a, **k)

    monkeypatch.setattr(S.QGraph, "detection_postprocess", with_scores_out)
    buf = S.efficientdet_lite2(np.int8, size=EDET_SIZE)
    monkeypatch.setattr(S.QGraph, "detection_postprocess", orig)
    om = OModel(buf)
    custom, deq = _dequant_ops(om)
    assert len(om.outputs) == 5 and custom.inputs[1] in om.outputs
    m, ex, key = _executor(buf, 45, monkeypatch)
    assert ex.PrepareSubgraph(m).ok()
    x = _edet()[2][0]
    ref = OracleInterpreter(om).run({om.inputs[0]: x})
    for rep in range(3):
        _run_and_compare(ex, key, om, x, ref, "run %d" % rep)
    launched = [r["op_index"] for r in ex.ProfileSubgraph(key, iters=1) if r["op_index"] in deq]
    assert launched == [i for i in deq if om.operators[i].outputs[0] == custom.inputs[1]]


def test_efficientdet_job_batches(gpu_lib, monkeypatch):
    buf, om, xs, refs = _edet()
    m, ex, key = _executor(buf, 46, monkeypatch)
    assert ex.PrepareSubgraph(m).ok()
    st = ex.PrepareJobBatches(m, key, 3)
    assert st.ok(), st.message()
    assert ex.MaxJobBatch(key) == 3
    for n, pick in ((2, (1, 2)), (3, (3, 0, 1)), (2, (0, 3))):
        for s, i in enumerate(pick):
            ex.GetJobSlotView(key, om.inputs[0], n, s).GetData()[...] = xs[i]
        assert ex.ExecuteJobBatch(key, n).ok()
        for s, i in enumerate(pick):
            for o in om.outputs:
                got = ex.GetJobSlotView(key, o, n, s).GetData()
                np.testing.assert_array_equal(got, refs[i][o].reshape(got.shape),
                                              err_msg="n=%d slot %d output %d" % (n, s, o))
    # a kCPU executor (knob on or not) keeps refusing to batch the model
    monkeypatch.setenv(KNOB, "1")
    cpu = HipModelExecutor(46, 0, DeviceFlag.kCPU, num_threads=2)
    assert cpu.PrepareSubgraph(m).ok()
    st = cpu.PrepareJobBatches(m, SubgraphKey(46, 0), 3)
    assert not st.ok() and "CUSTOM" in st.message()
    # ... and so does a kGPU executor without the knob, on its GPU part
    m0, ex0, _ = _executor(buf, 47, monkeypatch, knob=None)
    spec = ex0.InvestigateModelSpec(m0)
    gpu_ops = [i for i in range(spec.num_ops) if i not in spec.unsupported_ops[DeviceFlag.kGPU]][:5]
    assert ex0.PrepareSubgraph(m0, gpu_ops, [0]).ok()
    st = ex0.PrepareJobBatches(m0, SubgraphKey(47, 1, [0]), 3)
    assert not st.ok() and "CUSTOM" in st.message()


def test_ssd_mobilenet_v2_with_postprocess(gpu_lib, monkeypatch):
    buf = S.ssd_mobilenet_v2(np.int8, size=96, postprocess=True)
    om = OModel(buf)
    assert [op.builtin for op in om.operators[-3:]] == [6, 6, 32]
    m, ex, key = _executor(buf, 48, monkeypatch)
    assert ex.InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kGPU] == set()
    assert ex.PrepareSubgraph(m).ok()
    for x in _inputs(om, 2, 9) * 2:
        ref = OracleInterpreter(om).run({om.inputs[0]: x})
        assert int(ref[om.outputs[3]][0]) > 0
        _run_and_compare(ex, key, om, x, ref, "ssd")


def test_engine_gpu_workers_only(gpu_lib, monkeypatch, tmp_path):
    """[kGPU, kGPU], no CPU worker: without the knob nothing can place the
    postprocess unit; with it the whole model is one GPU subgraph"""
    monkeypatch.setenv(KNOB, "1")
    buf, om, xs, refs = _edet()
    path = str(tmp_path / "edet.tflite")
    with open(path, "wb") as f:
        f.write(buf)
    e = Engine(make_config([SchedulerType.kRoundRobin], [DeviceFlag.kGPU, DeviceFlag.kGPU]))
    m = Model()
    assert m.FromPath(path)
    assert e.RegisterModel(m)
    n_out = e.GetNumOutputTensors(m)
    assert n_out == 4
    ins = [e.CreateInputTensor(m, 0) for _ in range(3)]
    hs = []
    for t, x in zip(ins, xs):
        t.data()[...] = x
        hs.append(e.RequestAsync(m, [t]))
    assert all(h >= 0 for h in hs)
    for h, ref in zip(hs, refs):
        outs = [e.CreateOutputTensor(m, k) for k in range(n_out)]
        assert e.Wait(h, outs) == kBandOk
        assert e.GetJobRecord(h).status == JobStatus.kSuccess
        for k, t in enumerate(sorted(om.outputs)):
            np.testing.assert_array_equal(outs[k].data().reshape(-1), ref[t].reshape(-1), err_msg="output %d" % k)
    e.close()
