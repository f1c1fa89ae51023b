#!/usr/bin/env python3
"""The attention core as one launch (BAND_HIP_FUSED_ATTENTION=1) and as the
default launches.

Per model - encoder_block(196, 192, 3, 768) and attention_block at (heads,
tokens, head dim) = (4, 256, 36) and (12, 64, 64) - two kGPU executors in one
process, one built with the flag and one without, alternated: per round, the
end-to-end wall time of `iters` ExecuteSubgraph calls (replayed graph) and
TimeSubgraph's device time per pass; once, ProfileSubgraph's per-kernel lines.
Median and min - max over the rounds; the two forms' outputs are compared first.
Usage: python tools/attn_profile.py [--rounds 7] [--iters 2000] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLAG = "BAND_HIP_FUSED_ATTENTION"
CORE = ("attention_i8_kernel", "bmm_mfma_kernel", "softmax_kernel")


def stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.rounds >= 7, "at least 7 rounds"
    from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
    from band_amd.tflite_synth import attention_block, encoder_block
    from tests import encoder_models as E

    models = (("encoder_block(196, 192, 3, 768)", lambda: encoder_block(np.int8, tokens=196, dim=192, heads=3, hidden=768)),
              ("attention_block(heads 4, tokens 256, head dim 36)", lambda: attention_block(np.int8, tokens=256, dim=144, heads=4)),
              ("attention_block(heads 12, tokens 64, head dim 64)", lambda: attention_block(np.int8, tokens=64, dim=768, heads=12)))
    os.environ.pop("BAND_HIP_FUSION", None)
    res = {"rounds": args.rounds, "iters": args.iters, "models": {}}
    mid = 0
    for name, build in models:
        buf = build()
        x = E.model_input(buf, seed=1)
        forms = {}
        for tag, flag in (("fused", "1"), ("default", None)):
            if flag is None:
                os.environ.pop(FLAG, None)
            else:
                os.environ[FLAG] = flag
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
            mid += 1
        os.environ.pop(FLAG, None)
        outs = {t: ex.GetTensorView(key, ex.GetOutputs(key)[0]).GetData().copy() for t, (m, ex, key) in forms.items()}
        assert np.array_equal(outs["fused"], outs["default"]), "the two forms differ on " + name
        wall = {t: [] for t in forms}
        dev = {t: [] for t in forms}
        for _ in range(args.rounds):
            for t, (m, ex, key) in forms.items():
                t0 = time.perf_counter()
                for _ in range(args.iters):
                    ex.ExecuteSubgraph(key)
                wall[t].append(1e6 * (time.perf_counter() - t0) / args.iters)
                dev[t].append(ex.TimeSubgraph(key, iters=200))
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
            core = sum(v["us"] for k, v in per.items() if k in CORE or k.startswith("reindex"))
            entry[t] = {"launches": len(rows), "kernel_sum_us": round(sum(1e3 * r["ms"] for r in rows), 2),
                        "attention_core_us": round(core, 2), "kernels": per, "wall_us_per_pass": stats(wall[t]),
                        "device_us_per_pass": stats(dev[t])}
            print(name, t, json.dumps(entry[t]), flush=True)
        assert "attention_i8_kernel" in entry["fused"]["kernels"] and "attention_i8_kernel" not in entry["default"]["kernels"]
        res["models"][name] = entry
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
