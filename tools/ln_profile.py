#!/usr/bin/env python3
"""An encoder block with its LayerNorms as one launch each and as ten.

encoder_block(tokens, dim, heads, hidden) on two kGPU executors in one process,
one with every fusion and one with BAND_HIP_FUSION=nolayernorm, alternated:
per round, the end-to-end wall time of `iters` ExecuteSubgraph calls (replayed
graph) and TimeSubgraph's device time per pass; once, ProfileSubgraph's
per-kernel lines.  Median and min - max over the rounds; the two forms' outputs
are compared first.  Also, for information, bh_mean_rows beside bh_mean on the
same bytes: a [tokens][dim] tensor reduced over its last axis by both (bh_mean:
one lane walks a row), and MobileNet's [1, 7, 7, 1280] reduced over H, W by
bh_mean beside the same bytes as 1280 rows of 49 through bh_mean_rows (the
other layout, not the same op).
Usage: python tools/ln_profile.py [--rounds 7] [--iters 2000] [--out profiles/NAME.json]
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

LN_OPS = ("mean_rows_kernel", "eltwise_sqdiff_kernel", "eltwise_kernel", "lut_u8_kernel", "layernorm_i8_kernel")


def stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--tokens", type=int, default=196)
    ap.add_argument("--dim", type=int, default=192)
    ap.add_argument("--heads", type=int, default=3)
    ap.add_argument("--hidden", type=int, default=768)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi
    from band_amd.device import DeviceBuffer, Stream
    from band_amd.tflite_synth import encoder_block
    from tests import encoder_models as E

    buf = encoder_block(np.int8, tokens=args.tokens, dim=args.dim, heads=args.heads, hidden=args.hidden)
    x = E.model_input(buf, seed=1)
    forms = {}
    for mid, (tag, fusion) in enumerate((("fused", None), ("nolayernorm", "nolayernorm"))):
        if fusion is None:
            os.environ.pop("BAND_HIP_FUSION", None)
        else:
            os.environ["BAND_HIP_FUSION"] = fusion
        m = HipModel(mid)
        assert m.FromBuffer(buf).ok()
        ex = HipModelExecutor(mid, 1, DeviceFlag.kGPU)
        st = ex.PrepareSubgraph(m)
        assert st.ok(), st.message()
        key = SubgraphKey(mid, 1)
        ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = x
        for _ in range(3):
            assert ex.ExecuteSubgraph(key).ok()
        forms[tag] = (m, ex, key)
    os.environ.pop("BAND_HIP_FUSION", None)
    outs = {t: ex.GetTensorView(key, ex.GetOutputs(key)[0]).GetData().copy() for t, (m, ex, key) in forms.items()}
    assert np.array_equal(outs["fused"], outs["nolayernorm"]), "the two forms differ"

    res = {"model": "encoder_block(tokens=%d, dim=%d, heads=%d, hidden=%d)" % (args.tokens, args.dim, args.heads, args.hidden),
           "rounds": args.rounds, "iters": args.iters, "forms": {}}
    wall = {t: [] for t in forms}
    dev = {t: [] for t in forms}
    for _ in range(args.rounds):
        for t, (m, ex, key) in forms.items():
            t0 = time.perf_counter()
            for _ in range(args.iters):
                ex.ExecuteSubgraph(key)
            wall[t].append(1e6 * (time.perf_counter() - t0) / args.iters)
            dev[t].append(ex.TimeSubgraph(key, iters=200))
    for t, (m, ex, key) in forms.items():
        rows = ex.ProfileSubgraph(key, iters=20)
        per = {}
        for r in rows:
            k = per.setdefault(r["kernel"], {"launches": 0, "us": 0.0})
            k["launches"] += 1
            k["us"] += 1e3 * r["ms"]
        for k in per.values():
            k["us"] = round(k["us"], 2)
        res["forms"][t] = {"launches": len(rows), "kernel_sum_us": round(sum(1e3 * r["ms"] for r in rows), 2),
                           "layernorm_ops_us": round(sum(v["us"] for k, v in per.items() if k in LN_OPS), 2),
                           "kernels": per, "wall_us_per_pass": stats(wall[t]), "device_us_per_pass": stats(dev[t])}
        print(t, json.dumps(res["forms"][t]), flush=True)

    # bh_mean_rows beside bh_mean, for information
    lib = _abi.load()
    st = Stream()
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        _abi.check(lib.bh_event_create(ctypes.byref(e)), "event")

    def timed(fn, iters=500):
        for _ in range(10):
            _abi.check(fn(), "launch")
        lib.bh_event_record(ev[0], st.handle)
        for _ in range(iters):
            fn()
        lib.bh_event_record(ev[1], st.handle)
        st.sync()
        ms = ctypes.c_float(0)
        _abi.check(lib.bh_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)), "elapsed")
        return 1e3 * ms.value / iters

    res["mean"] = {}
    rng = np.random.default_rng(5)
    for name, (outer, reduce, inner), (rows, depth) in (("last_axis_%dx%d" % (args.tokens, args.dim), (args.tokens, args.dim, 1),
                                                         (args.tokens, args.dim)),
                                                        ("hw_1x7x7x1280", (1, 49, 1280), (1280, 49))):
        data = rng.integers(-128, 128, outer * reduce * inner).astype(np.int8)
        dx, dy = DeviceBuffer.from_array(data), DeviceBuffer(max(outer * inner, rows))
        pm = _abi.MeanParams()
        pm.outer, pm.reduce, pm.inner, pm.type = outer, reduce, inner, 1
        pm.multiplier, pm.shift, pm.bias = 1 << 30, -5, 0
        pm.input, pm.output = dx.value, dy.value
        pr = _abi.MeanRowsParams()
        pr.rows, pr.depth, pr.type, pr.exact, pr.scale, pr.bias, pr.out_zp = rows, depth, 1, 0, 0.7, 0.5, 0
        pr.input, pr.output = dx.value, dy.value
        us = {"mean_kernel": [], "mean_rows_kernel": []}
        for _ in range(args.rounds):
            us["mean_kernel"].append(timed(lambda: lib.bh_mean(ctypes.byref(pm), st.handle)))
            us["mean_rows_kernel"].append(timed(lambda: lib.bh_mean_rows(ctypes.byref(pr), st.handle)))
        res["mean"][name] = {k: stats(v) for k, v in us.items()}
        print(name, json.dumps(res["mean"][name]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
