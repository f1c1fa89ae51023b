#!/usr/bin/env python3
"""Hybrid FULLY_CONNECTED (float32 input, int8 weights: dynquant_rows_kernel +
fc_hybrid_kernel) against the float32 FULLY_CONNECTED of the fp16-constant
model (fc_f32_kernel).

Two pairs of models, each as float32 with fp16 constants and as the hybrid
(asymmetric) model: encoder_block(196, 192, 3, 768), and a 1 x 1280 -> 1001
classifier head.  Per pair two kGPU executors in one process, alternated: per
round TimeSubgraph's device time per pass (replayed graph) and the end-to-end
wall time of `iters` ExecuteSubgraph calls; once, ProfileSubgraph's per-kernel
lines.  Median and min - max over the rounds.  The two forms compute different
functions (the hybrid one quantises), so their outputs are not compared here;
tests/test_fc_hybrid_gpu.py holds the hybrid values.
Usage: python tools/fc_hybrid_profile.py [--rounds 7] [--iters 1000] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FC_KERNELS = ("fc_f32_kernel", "dynquant_rows_kernel", "fc_hybrid_kernel")


def stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}


def head(hybrid):
    from band_amd.tflite_synth import FGraph
    g = FGraph(seed=3, name="head_1280_1001", hybrid=hybrid)
    g.output(g.fully_connected(g.input([1, 1280]), 1001))
    return g.build()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--hybrid", default="asymmetric", choices=("symmetric", "asymmetric"))
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.rounds >= 7, "at least 7 rounds"
    from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
    from band_amd.tflite_synth import encoder_block

    pairs = (("encoder_block(196, 192, 3, 768)",
              lambda hy: encoder_block(np.float32, tokens=196, dim=192, heads=3, hidden=768, hybrid=hy)),
             ("head 1 x 1280 -> 1001", head))
    os.environ.pop("BAND_HIP_FUSION", None)
    res = {"rounds": args.rounds, "iters": args.iters, "hybrid": args.hybrid, "models": {}}
    mid = 0
    for name, build in pairs:
        forms = {}
        for tag, hy in (("hybrid", args.hybrid), ("float32_fp16_constants", None)):
            buf = build(hy)
            m = HipModel(mid)
            assert m.FromBuffer(buf).ok()
            ex = HipModelExecutor(mid, 1, DeviceFlag.kGPU)
            st = ex.PrepareSubgraph(m)
            assert st.ok(), st.message()
            key = SubgraphKey(mid, 1)
            view = ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()
            view[...] = np.random.default_rng(1).normal(0, 1, view.shape)
            for _ in range(3):
                assert ex.ExecuteSubgraph(key).ok()
            assert np.isfinite(ex.GetTensorView(key, ex.GetOutputs(key)[0]).GetData()).all()
            forms[tag] = (m, ex, key)
            mid += 1
        wall = {t: [] for t in forms}
        dev = {t: [] for t in forms}
        for _ in range(args.rounds):
            for t, (m, ex, key) in forms.items():
                dev[t].append(ex.TimeSubgraph(key, iters=200))
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    ex.ExecuteSubgraph(key)
                wall[t].append(1e6 * (time.perf_counter() - t0) / args.iters)
        entry = {}
        for t, (m, ex, key) in forms.items():
            rows = ex.ProfileSubgraph(key, iters=20)
            per = {}
            for r in rows:
                k = per.setdefault(r["kernel"], {"launches": 0, "us": 0.0})
                k["launches"] += 1
                k["us"] += 1e3 * r["ms"]
            for k in per.values():
                k["us"] = round(k["us"], 2)
            total = sum(1e3 * r["ms"] for r in rows)
            fc = sum(v["us"] for k, v in per.items() if k in FC_KERNELS)
            entry[t] = {"launches": len(rows), "kernel_sum_us": round(total, 2), "fully_connected_us": round(fc, 2),
                        "fully_connected_share": round(fc / total, 3) if total else 0.0, "kernels": per,
                        "device_us_per_pass": stats(dev[t]), "wall_us_per_pass": stats(wall[t])}
            print(name, t, json.dumps(entry[t]), flush=True)
        assert "fc_hybrid_kernel" in entry["hybrid"]["kernels"] and "dynquant_rows_kernel" in entry["hybrid"]["kernels"]
        assert "fc_f32_kernel" in entry["float32_fp16_constants"]["kernels"]
        res["models"][name] = entry
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
