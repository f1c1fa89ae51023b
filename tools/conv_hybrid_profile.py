#!/usr/bin/env python3
"""Hybrid CONV_2D / DEPTHWISE_CONV_2D (float32 input, int8 filter: the item
quantisation, then conv_hybrid_kernel / dwconv_hybrid_kernel) against the
float32 convolutions of the fp16-constant model (conv_f32_kernel /
dwconv_f32_kernel).

Models: mobilenet_v2 and mobilenet_v1 at 224, at batch 1 and at batch 8, and
the patch conv of vit_tiny(224); each as the dynamic-range model (per-channel
filters, on an executor built with BAND_HIP_HYBRID_CONV=1) and as the float32
model with fp16 constants, which runs none of the new kernels.  Batch 8 is the
models' own batch axis: an fp16-constant graph has no job-batch variants (its
DEQUANTIZE outputs have no batch axis), so the two forms can only be laid side
by side that way; the hybrid model's job batch of 8 is timed beside it (wall
time per ExecuteJobBatch).

Per pair two kGPU executors in one process.  First the outputs are checked: the
hybrid executor's every op against the rule (exact) and the float bound, the
float executor's every op against the float bound (tests/hybrid_conv_models.py,
tests/float_harness.py).  Then, alternated over the rounds, TimeSubgraph's device
time per pass (replayed graph) and the wall time of `iters` ExecuteSubgraph
calls; once, ProfileSubgraph's per-kernel lines, summed per kernel and per
convolution (the n-th CONV_2D / DEPTHWISE_CONV_2D of either graph), so that the
layers where the hybrid launches lose to the one float launch are listed.
Median and min - max over the rounds.

Beside the models, once each with dispatch timestamps (median of 21):
bh_dynquant_items in its one-launch and its two-launch form on items around
BH_DYNQUANT_ONE_LAUNCH_MAX, and conv_hybrid_kernel on the 1 x 1 layer
[196 x 768] -> 192 beside bh_fc_hybrid on the same bytes.
Usage: python tools/conv_hybrid_profile.py [--rounds 7] [--iters 300] [--out profiles/NAME.json]
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CONV_KERNELS = ("conv_f32_kernel", "dwconv_f32_kernel", "dynquant_item_kernel",
                "dynquant_minmax_kernel+dynquant_items_kernel", "conv_hybrid_kernel", "dwconv_hybrid_kernel")


def stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}


def patch_conv(hybrid_conv, size=224, dim=192):
    from band_amd.tflite_synth import FGraph
    g = FGraph(seed=7, name="vit_patch_conv", hybrid_conv=hybrid_conv)
    g.output(g.conv(g.input([1, size, size, 3]), dim, k=16, stride=16, act="NONE", padding="VALID"))
    return g.build()


def timed(lib, run, reps=21):
    """median dispatch-timestamp duration (us) of run(), first kernel's begin to last kernel's end"""
    from band_amd import _abi
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        _abi.check(lib.bh_event_create(ctypes.byref(e)), "bh_event_create")
    out = []
    for _ in range(reps + 3):
        lib.bh_profile_events(ev[0], ev[1])
        run()
        lib.bh_profile_events(None, None)
        _abi.check(lib.bh_event_sync(ev[1]), "bh_event_sync")
        ms = ctypes.c_float(0)
        _abi.check(lib.bh_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)), "bh_event_elapsed_ms")
        out.append(1e3 * ms.value)
    for e in ev:
        lib.bh_event_destroy(e)
    return round(sorted(out[3:])[reps // 2], 2)


def launcher_timings(lib):
    """the quantiser's two forms around the crossover, and the 1 x 1 layer beside bh_fc_hybrid"""
    from band_amd import _abi
    from tests import hybrid_conv_models as C
    from tests import hybrid_models as Y
    res = {"dynquant_items_us": {}, "pointwise_196x768_to_192_us": {}}
    for size in (4096, 8192, 16384, 32768, 65536, 150528, 1204224):
        x = np.random.default_rng(size).normal(0, 1, (1, size)).astype(np.float32)
        o = C._Outputs(True)
        row = {}
        for form, tag in ((1, "one_launch"), (2, "two_launches")):
            p, _, _, _ = C._dq_block(o, x, True, form, 0, 0)
            row[tag] = timed(lib, lambda: _abi.check(lib.bh_dynquant_items(ctypes.byref(p), None), "bh_dynquant_items"))
        res["dynquant_items_us"][str(size)] = row
        print("dynquant_items", size, json.dumps(row), flush=True)
    case = C.ConvCase("pt", 1, (14, 14), 768, 192, 1, seed=1)
    o = C._Outputs(True)
    p, _, _, _ = C._dq_block(o, case.x.reshape(1, -1), False, 0, 0, 0)
    _abi.check(lib.bh_dynquant_items(ctypes.byref(p), None), "bh_dynquant_items")
    packed, k_pad, sums = C.pack_filter(case)
    dy = o.out(4 * case.M * case.out_c, 0, C.NAN_WORD)
    keep = [C.buffer(a, True) for a in (packed, sums, case.ws, case.bias)]
    f = C.conv_block(case, dict(q=p.q, in_scale=p.scale, in_offset=p.offset, weights=keep[0].value, w_row_sum=keep[1].value,
                                w_scale=keep[2].value, bias=keep[3].value, output=dy.value))
    f.k_pad = k_pad
    res["pointwise_196x768_to_192_us"]["conv_hybrid_kernel"] = timed(
        lib, lambda: _abi.check(lib.bh_conv2d_hybrid(ctypes.byref(f), None), "bh_conv2d_hybrid"))
    # the same bytes as 196 rows of depth 768: per-row scales and offsets (196 copies of the item's)
    rows = 196
    ds = C.buffer(np.full(rows, 0.01, np.float32), True)
    do = C.buffer(np.zeros(rows, np.int32), True)
    h = _abi.FcHybridParams()
    h.rows, h.depth, h.depth_pad, h.units = rows, 768, 768, 192
    h.w_scale, (h.act_min, h.act_max) = 0.0123, Y.H.ACT["NONE"]
    h.q, h.in_scale, h.in_offset = p.q, ds.value, do.value
    h.weights, h.w_row_sum, h.bias, h.output = keep[0].value, keep[1].value, keep[3].value, dy.value
    res["pointwise_196x768_to_192_us"]["fc_hybrid_kernel"] = timed(
        lib, lambda: _abi.check(lib.bh_fc_hybrid(ctypes.byref(h), None), "bh_fc_hybrid"))
    print("pointwise", json.dumps(res["pointwise_196x768_to_192_us"]), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.rounds >= 7, "at least 7 rounds"
    from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi
    from band_amd.tflite_synth import mobilenet_v1, mobilenet_v2
    from oracle.tflite_fb import Model as OModel
    from tests import float_harness as H
    from tests import hybrid_conv_models as C

    def pair(fn, batch):
        return lambda hc: (fn(np.float32, size=args.size, batch=batch, hybrid_conv=hc) if hc else
                           fn(np.float16, size=args.size, batch=batch))
    pairs = [("mobilenet_v2 batch 1", pair(mobilenet_v2, 1), 8), ("mobilenet_v2 batch 8", pair(mobilenet_v2, 8), 0),
             ("mobilenet_v1 batch 1", pair(mobilenet_v1, 1), 8), ("mobilenet_v1 batch 8", pair(mobilenet_v1, 8), 0),
             ("vit_tiny patch conv", lambda hc: patch_conv(hc, args.size), 0)]
    os.environ.pop("BAND_HIP_FUSION", None)
    res = {"rounds": args.rounds, "iters": args.iters, "size": args.size, "models": {}}
    mid = 0
    for name, build, job_batch in pairs:
        forms = {}
        for tag, hc in (("hybrid", "per_channel"), ("float32_fp16_constants", None)):
            buf = build(hc)
            om = OModel(buf)
            feed = C.model_feed(buf, seed=1)
            # the values first: every op of a run with every tensor viewed
            os.environ["BAND_HIP_HYBRID_CONV"] = "1" if hc else "0"
            _, runs = H.run_executor(buf, [feed], DeviceFlag.kGPU, 1, view_all=True)
            n = H.check_graph_ops(om, runs[0], name + " " + tag, gelu_ulps=16)[1]["conv"]
            assert (n > 0) == bool(hc), (name, tag, n)
            m = HipModel(mid)
            assert m.FromBuffer(buf).ok()
            ex = HipModelExecutor(mid, 1, DeviceFlag.kGPU)
            st = ex.PrepareSubgraph(m)
            assert st.ok(), st.message()
            key = SubgraphKey(mid, 1)
            ex.GetTensorView(key, om.inputs[0]).GetData()[...] = feed[om.inputs[0]]
            for _ in range(3):
                assert ex.ExecuteSubgraph(key).ok()
            got = ex.GetTensorView(key, om.outputs[0]).GetData()
            np.testing.assert_array_equal(got.reshape(runs[0][om.outputs[0]].shape), runs[0][om.outputs[0]])
            convs = [i for i, o in enumerate(om.operators) if o.builtin in (C.CONV_2D, C.DEPTHWISE_CONV_2D)]
            forms[tag] = (m, ex, key, om, convs)
            mid += 1
        wall = {t: [] for t in forms}
        dev = {t: [] for t in forms}
        for _ in range(args.rounds):
            for t, (m, ex, key, om, convs) in forms.items():
                dev[t].append(ex.TimeSubgraph(key, iters=100))
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    ex.ExecuteSubgraph(key)
                wall[t].append(1e6 * (time.perf_counter() - t0) / args.iters)
        entry, per_conv = {}, {}
        for t, (m, ex, key, om, convs) in forms.items():
            rows = ex.ProfileSubgraph(key, iters=20)
            per = {}
            for r in rows:
                k = per.setdefault(r["kernel"], {"launches": 0, "us": 0.0})
                k["launches"] += 1
                k["us"] += 1e3 * r["ms"]
            for k in per.values():
                k["us"] = round(k["us"], 2)
            total = sum(1e3 * r["ms"] for r in rows)
            conv_us = sum(v["us"] for k, v in per.items() if k.split("+add")[0] in CONV_KERNELS or k in CONV_KERNELS)
            per_conv[t] = [round(sum(1e3 * r["ms"] for r in rows if r["op_index"] == i), 2) for i in convs]
            entry[t] = {"launches": len(rows), "kernel_sum_us": round(total, 2), "convolutions_us": round(conv_us, 2),
                        "kernels": per, "device_us_per_pass": stats(dev[t]), "wall_us_per_pass": stats(wall[t])}
            print(name, t, json.dumps(entry[t]), flush=True)
        m, ex, key, om, convs = forms["hybrid"]
        layers = []
        for n, i in enumerate(convs):
            o = om.operators[i]
            layers.append({"conv": n, "op": o.name, "input": om.tensors[o.inputs[0]].shape, "filter": om.tensors[o.inputs[1]].shape,
                           "hybrid": C.is_hybrid_conv(om, o), "hybrid_us": per_conv["hybrid"][n],
                           "float_us": per_conv["float32_fp16_constants"][n]})
        entry["layers"] = layers
        lost = [ly for ly in layers if ly["hybrid"] and ly["hybrid_us"] > ly["float_us"]]
        entry["hybrid_layers"] = sum(ly["hybrid"] for ly in layers)
        entry["hybrid_layers_slower_than_float"] = [ly["conv"] for ly in lost]
        print(name, "hybrid layers", entry["hybrid_layers"], "of which slower than the float launch", len(lost), flush=True)
        if job_batch:
            os.environ["BAND_HIP_HYBRID_CONV"] = "1"
            st = ex.PrepareJobBatches(m, key, job_batch)
            assert st.ok(), st.message()
            for s in range(job_batch):
                ex.GetJobSlotView(key, om.inputs[0], job_batch, s).GetData()[...] = C.model_feed(om.buf, seed=s)[om.inputs[0]]
            for _ in range(3):
                assert ex.ExecuteJobBatch(key, job_batch).ok()
            jw = []
            for _ in range(args.rounds):
                t0 = time.perf_counter()
                for _ in range(max(1, args.iters // 4)):
                    ex.ExecuteJobBatch(key, job_batch)
                jw.append(1e6 * (time.perf_counter() - t0) / max(1, args.iters // 4))
            entry["hybrid_job_batch_%d_wall_us" % job_batch] = stats(jw)
            print(name, "job batch", job_batch, json.dumps(stats(jw)), flush=True)
        res["models"][name] = entry
    res.update(launcher_timings(_abi.load()))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
