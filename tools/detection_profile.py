#!/usr/bin/env python3
"""Device time of the detection postprocess kernels (kernels/detection.hip)
on EfficientDet-Lite2's real head outputs.

  1. The model whole on one kGPU executor with BAND_HIP_GPU_DETECTION=1:
     ProfileSubgraph's row of detection_postprocess_kernel (per-dispatch
     begin / end timestamps, both kernels of the launcher) next to the sum
     of all launches of a pass.
  2. bh_detection_postprocess called directly on that pass's 8-bit box
     encodings and class scores, replicated to a batch of B images, timed by
     events around `--iters` back-to-back launches: batch 1 and --batch.

Prints one JSON line.  Usage: python tools/detection_profile.py [--size 448]
[--batch 8] [--iters 50]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ["BAND_HIP_GPU_DETECTION"] = "1"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=448)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    import band_amd
    from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi, tflite_synth as S
    from band_amd.device import DeviceBuffer, Stream
    from oracle.detection_postprocess import read_flexbuffer_map
    from oracle.tflite_fb import Model as OModel

    buf = S.efficientdet_lite2(np.int8, size=args.size)
    om = OModel(buf)
    custom = next(op for op in om.operators if op.builtin == 32)
    opts = read_flexbuffer_map(custom.custom_options)
    q = {}  # box encodings / class scores: the 8-bit inputs of the two DEQUANTIZEs
    for k, t in enumerate(custom.inputs[:2]):
        deq = next(op for op in om.operators if op.builtin == 6 and op.outputs[0] == t)
        q[k] = deq.inputs[0]
    band_amd.SetWorkerDevice(1, 0)
    m = HipModel(0)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(0, 1, DeviceFlag.kGPU)
    assert ex.InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kGPU] == set()
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(0, 1)
    x = np.random.default_rng(0).integers(-128, 128, (1, args.size, args.size, 3)).astype(np.int8)
    ex.GetTensorView(key, om.inputs[0]).GetData()[...] = x
    for _ in range(3):
        assert ex.ExecuteSubgraph(key).ok()
    num = float(ex.GetTensorView(key, om.outputs[3]).GetData().reshape(-1)[0])
    ex.TimeSubgraph(key, iters=20)
    pass_us = ex.TimeSubgraph(key, iters=100)
    rows = ex.ProfileSubgraph(key, iters=args.iters)
    det = [r for r in rows if r["kernel"] == "detection_postprocess_kernel"]
    assert len(det) == 1
    out = {"model": "efficientdet_lite2_int8", "size": args.size, "anchors": om.tensors[custom.inputs[2]].shape[0],
           "detections": num,
           "executor_batch1": {"detection_us": det[0]["ms"] * 1e3, "alg_bytes": det[0]["alg_bytes"],
                               "all_launches_us": sum(r["ms"] for r in rows) * 1e3, "launches": len(rows),
                               "device_us_per_pass": pass_us}}
    # the same model without the knob: the GPU part of the split (the ops
    # before the CPU-only ones), as the analyzer places it
    os.environ["BAND_HIP_GPU_DETECTION"] = "0"
    m_off = HipModel(1)
    assert m_off.FromBuffer(buf).ok()
    ex_off = HipModelExecutor(1, 1, DeviceFlag.kGPU)
    spec = ex_off.InvestigateModelSpec(m_off)
    gpu_ops = [i for i in range(spec.num_ops) if i not in spec.unsupported_ops[DeviceFlag.kGPU]]
    assert len(gpu_ops) == spec.num_ops - 3 and ex_off.PrepareSubgraph(m_off, gpu_ops).ok()
    key_off = SubgraphKey(1, 1)
    ex_off.GetTensorView(key_off, om.inputs[0]).GetData()[...] = x
    ex_off.TimeSubgraph(key_off, iters=20)
    rows_off = ex_off.ProfileSubgraph(key_off, iters=args.iters)
    out["split_gpu_part_batch1"] = {"device_us_per_pass": ex_off.TimeSubgraph(key_off, iters=100),
                                    "all_launches_us": sum(r["ms"] for r in rows_off) * 1e3,
                                    "launches": len(rows_off)}
    os.environ["BAND_HIP_GPU_DETECTION"] = "1"
    # the pass's 8-bit head outputs, for the launcher timing below
    views = {k: ex.GetTensorView(key, t) for k, t in q.items()}
    assert ex.ExecuteSubgraph(key).ok()

    lib = _abi.load()
    anchors = np.ascontiguousarray(om.tensors[custom.inputs[2]].data, np.float32)
    n, d = anchors.shape[0], int(opts["max_detections"])
    be1 = np.ascontiguousarray(views[0].GetData()).reshape(n, 4).copy()
    cs1 = np.ascontiguousarray(views[1].GetData()).reshape(n, -1).copy()
    tq = [om.tensors[q[0]], om.tensors[q[1]]]
    score = np.float32(tq[1].scale[0]) * (cs1.astype(np.int32).max(axis=1) - int(tq[1].zero_point[0]))
    out["candidates"] = int((score >= np.float32(opts["nms_score_threshold"])).sum())
    stream = Stream()
    d_an = DeviceBuffer.from_array(anchors)
    launcher = {}
    for b in sorted({1, args.batch}):
        d_be = DeviceBuffer.from_array(np.tile(be1[None], (b, 1, 1)))
        d_cs = DeviceBuffer.from_array(np.tile(cs1[None], (b, 1, 1)))
        scratch = DeviceBuffer(lib.bh_detection_scratch_bytes(b, n))
        outs = [DeviceBuffer(4 * b * k) for k in (d * 4, d, d, 1)]
        p = _abi.DetectionParams(
            batch=b, num_boxes=n, num_classes=int(opts["num_classes"]), num_classes_with_background=cs1.shape[1],
            max_detections=d, score_threshold=opts["nms_score_threshold"], iou_threshold=opts["nms_iou_threshold"],
            scale_y=opts["y_scale"], scale_x=opts["x_scale"], scale_h=opts["h_scale"], scale_w=opts["w_scale"],
            box_type=1, score_type=1, box_scale=float(tq[0].scale[0]), score_scale=float(tq[1].scale[0]),
            box_zp=int(tq[0].zero_point[0]), score_zp=int(tq[1].zero_point[0]), box_encodings=d_be.value,
            class_scores=d_cs.value, anchors=d_an.value, out_boxes=outs[0].value, out_classes=outs[1].value,
            out_scores=outs[2].value, out_num=outs[3].value, scratch=scratch.value)
        e0, e1 = ctypes.c_void_p(), ctypes.c_void_p()
        _abi.check(lib.bh_event_create(ctypes.byref(e0)), "event")
        _abi.check(lib.bh_event_create(ctypes.byref(e1)), "event")
        for timed in (False, True):  # one untimed round first
            lib.bh_event_record(e0, stream.handle)
            for _ in range(args.iters):
                _abi.check(lib.bh_detection_postprocess(ctypes.byref(p), stream.handle), "bh_detection_postprocess")
            lib.bh_event_record(e1, stream.handle)
            stream.sync()
        ms = ctypes.c_float(0)
        _abi.check(lib.bh_event_elapsed_ms(e0, e1, ctypes.byref(ms)), "elapsed")
        got_num = outs[3].download(np.float32, (b,))
        assert (got_num == num).all(), (got_num, num)
        launcher["batch_%d" % b] = {"us_per_launch": ms.value * 1e3 / args.iters,
                                    "us_per_image": ms.value * 1e3 / args.iters / b}
        lib.bh_event_destroy(e0)
        lib.bh_event_destroy(e1)
    out["launcher_8bit"] = launcher
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
