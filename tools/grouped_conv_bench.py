#!/usr/bin/env python3
"""Device time of grouped CONV_2D layers beside the same layer written as
SPLIT -> G x CONV_2D -> CONCATENATION (what a model had to be rewritten to
before the backend accepted groups).

Layers: ShuffleNet-v1 g=3 at 224 (the two grouped 1x1 layers of a unit in
stages 2-4) and the 3x3 of a ResNeXt-50 32x4d block at 56 / 28 / 14 / 7, at
batch 1 and 24.  Per layer two int8 one-layer models on a kGPU executor:
  grouped   x -> CONV_2D (groups = G), one conv_grouped_mfma_kernel launch
  split     x -> SPLIT -> G x CONV_2D -> CONCATENATION (in trees of <= 16
            inputs), RELU6 everywhere so no branch needs a requantise
alternated inside one process: per round each model's ProfileSubgraph (kernel
begin / end timestamps of every launch, summed: no launch gaps) and
TimeSubgraph (graph replay per pass, host copies included).  Then the launcher
alone, each form pinned by kernel_hint (conv_grouped_mfma_kernel with one and
with two 16-pixel tiles per wave) beside the routed one: `iters` launches back
to back between two events, so each figure holds one dispatch.  Median and
min - max over the rounds; `spread` is max - min of the grouped model.
Usage: python tools/grouped_conv_bench.py [--rounds 5] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (name, spatial, in_c, out_c, k, groups)
LAYERS = [
    ("shufflenet_s2_pw1", 28, 240, 60, 1, 3), ("shufflenet_s2_pw2", 28, 60, 240, 1, 3),
    ("shufflenet_s3_pw1", 14, 480, 120, 1, 3), ("shufflenet_s3_pw2", 14, 120, 480, 1, 3),
    ("shufflenet_s4_pw1", 7, 960, 240, 1, 3), ("shufflenet_s4_pw2", 7, 240, 960, 1, 3),
    ("resnext_56", 56, 128, 128, 3, 32), ("resnext_28", 28, 256, 256, 3, 32),
    ("resnext_14", 14, 512, 512, 3, 32), ("resnext_7", 7, 1024, 1024, 3, 32),
]


def grouped_model(batch, hw, ic, oc, k, groups):
    from band_amd.tflite_synth import QGraph
    g = QGraph(np.int8, seed=11, name="grouped")
    x = g.input([batch, hw, hw, ic], scale=0.05)
    g.output(g.conv(x, oc, k=k, groups=groups))
    return g.build()


def split_model(batch, hw, ic, oc, k, groups):
    from band_amd.tflite_synth import QGraph
    g = QGraph(np.int8, seed=11, name="split")
    x = g.input([batch, hw, hw, ic], scale=0.05)
    ys = [g.conv(p, oc // groups, k=k) for p in g.split(x, groups, axis=3)]
    while len(ys) > 16:  # CONCATENATION takes up to 16 inputs
        ys = [g.concat(ys[i:i + 16], axis=3) for i in range(0, len(ys), 16)]
    g.output(g.concat(ys, axis=3) if len(ys) > 1 else ys[0])
    return g.build()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", help="substring a layer's name must contain")
    args = ap.parse_args()
    from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey

    def prepare(buf, mid):
        m = HipModel(mid)
        assert m.FromBuffer(buf).ok()
        ex = HipModelExecutor(mid, 1, DeviceFlag.kGPU)
        st = ex.PrepareSubgraph(m)
        assert st.ok(), st.message()
        key = SubgraphKey(mid, 1)
        ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = 3
        for _ in range(3):  # eager pass, graph capture, one replay
            assert ex.ExecuteSubgraph(key).ok()
        return m, ex, key

    import ctypes
    from band_amd import _abi
    from band_amd.device import Stream
    from tests import grouped_models as G
    lib = _abi.load()
    stream = Stream()
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        _abi.check(lib.bh_event_create(ctypes.byref(e)), "event")

    def forms(batch, hw, ic, oc, k, groups):
        """us per launch of bh_conv2d_grouped_i8: routed, and each pixel tile pinned"""
        case = G.GroupedCase((batch, hw, hw, groups, ic // groups, oc // groups, k, k, 1, 1, True), np.int8,
                             act=G.RELU6, seed=5)
        keep = []
        p = G.grouped_params(case, lib, keep, True)
        us = {"routed": [], "tile1": [], "tile2": []}
        hint = {"routed": 0, "tile1": G.MFMA, "tile2": G.MFMA_2}
        for _ in range(args.rounds):
            for v in us:
                p.conv.kernel_hint = hint[v]
                for _ in range(10):
                    _abi.check(lib.bh_conv2d_grouped_i8(ctypes.byref(p), stream.handle), "launch")
                lib.bh_event_record(ev[0], stream.handle)
                for _ in range(10 * args.iters):
                    lib.bh_conv2d_grouped_i8(ctypes.byref(p), stream.handle)
                lib.bh_event_record(ev[1], stream.handle)
                stream.sync()
                ms = ctypes.c_float(0)
                _abi.check(lib.bh_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)), "elapsed")
                us[v].append(1e3 * ms.value / (10 * args.iters))
        return {v: stats(t) for v, t in us.items()}

    def stats(v):
        s = sorted(v)
        return {"us_median": round(s[len(s) // 2], 2), "us_min": round(s[0], 2), "us_max": round(s[-1], 2)}

    res = {"rounds": args.rounds, "iters": args.iters, "layers": {}}
    mid = 100
    for name, hw, ic, oc, k, groups in LAYERS:
        if args.only not in name:
            continue
        for batch in (1, 24):
            models = {"grouped": prepare(grouped_model(batch, hw, ic, oc, k, groups), mid),
                      "split": prepare(split_model(batch, hw, ic, oc, k, groups), mid + 1)}
            mid += 2
            kern = {v: [] for v in models}
            full = {v: [] for v in models}
            launches = {}
            for _ in range(args.rounds):
                for v, (m, ex, key) in models.items():
                    rows = ex.ProfileSubgraph(key, iters=args.iters)
                    launches[v] = [r["kernel"] for r in rows]
                    kern[v].append(1e3 * sum(r["ms"] for r in rows))
                    full[v].append(ex.TimeSubgraph(key, iters=5 * args.iters))
            row = {"batch": batch, "groups": groups, "k_g": k * k * ic // groups,
                   "grouped_kernel": launches["grouped"], "split_launches": len(launches["split"])}
            for v in models:
                row[v] = {"kernels": stats(kern[v]), "pass": stats(full[v])}
            for what in ("kernels", "pass"):
                a, b = row["grouped"][what], row["split"][what]
                row["%s_speedup" % what] = round(b["us_median"] / a["us_median"], 2)
                row["%s_gain_us" % what] = round(b["us_median"] - a["us_median"], 2)
                row["%s_spread_us" % what] = round(a["us_max"] - a["us_min"], 2)
            row["forms"] = forms(batch, hw, ic, oc, k, groups)
            res["layers"]["%s_b%d" % (name, batch)] = row
            print("%s_b%d" % (name, batch), json.dumps(row), flush=True)
            del models
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
