#!/usr/bin/env python3
"""The float32 LayerNorm as one launch that also quantises its rows
(BAND_HIP_FUSED_LAYERNORM_F32=1: layernorm_f32_kernel) against the ten
launches plus one dynquant_rows_kernel per hybrid FULLY_CONNECTED.

One process, two kGPU executors of encoder_block(float32, 196, 192, 3, 768,
hybrid="asymmetric"), one built with the variable set and one without.  First
the fused form's values are checked as tests/test_layernorm_f32_gpu.py checks
them: on the same block with the Q, K and V projections as extra outputs, the
four projections that read a LayerNorm must equal the rule bit for bit.  Then
the two executors are alternated: per round TimeSubgraph's device time per
pass (replayed graph) and the wall time of `iters` ExecuteSubgraph calls; once,
ProfileSubgraph's per-kernel sums.  Median and min - max over the rounds.
Usage: python tools/ln_f32_profile.py [--rounds 7] [--iters 1000] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FLAG = "BAND_HIP_FUSED_LAYERNORM_F32"
SHAPE = (196, 192, 3, 768)
LN_KERNELS = ("layernorm_f32_kernel", "mean_kernel", "eltwise_f32_kernel", "unary_f32_kernel", "dynquant_rows_kernel")


def stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}


def executor(buf, mid, fused):
    from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
    if fused:
        os.environ[FLAG] = "1"
    else:
        os.environ.pop(FLAG, None)
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(mid, 1, DeviceFlag.kGPU)
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    os.environ.pop(FLAG, None)
    return m, ex, SubgraphKey(mid, 1)


def check_values():
    """the projections that read the two LayerNorms, bit for bit against the rule; returns how many were compared"""
    from oracle.tflite_fb import Model as OModel
    from tests import hybrid_models as Y
    from tests import layernorm_f32_models as L
    buf = L.encoder_with_qkv_outputs("asymmetric", SHAPE)
    om = OModel(buf)
    lns = L.layer_norms(om)
    fcs = [o for o in om.operators if Y.is_hybrid_fc(om, o)]
    readers = [[o for o in fcs if o.inputs[0] == ln[4]] for ln in lns]
    assert [len(r) for r in readers] == [3, 1]
    m, ex, key = executor(buf, 90, True)
    kernels = ex.LaunchKernels(key)
    assert len(kernels) == 20 and kernels.count("layernorm_f32_kernel") == 2, kernels
    want = list(om.outputs) + [lns[1][0], readers[1][0].outputs[0]]
    views = {t: ex.GetTensorView(key, t) for t in want}
    feed = Y.model_feed(buf, seed=1)
    n = 0
    for _ in range(3):  # eager, capture, replay
        for t in om.inputs:
            ex.GetTensorView(key, t).GetData()[...] = feed[t]
        assert ex.ExecuteSubgraph(key).ok()
        vals = {t: v.GetData().copy() for t, v in views.items()}
        vals[om.inputs[0]] = feed[om.inputs[0]]
        for ln, rd in zip(lns, readers):
            y = L.model_layernorm(om, ln, vals[ln[0]])
            for o in rd:
                ref = L.fc_from_rows(om, o, y)
                got = vals[o.outputs[0]].reshape(ref.shape)
                assert (got.view(np.uint32) == ref.view(np.uint32)).all(), "projection %d differs from the rule" % o.outputs[0]
                n += 1
    return n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.rounds >= 7, "at least 7 rounds"
    from band_amd.tflite_synth import encoder_block

    os.environ.pop("BAND_HIP_FUSION", None)
    checked = check_values()
    print("values: %d projections equal the rule bit for bit" % checked, flush=True)
    t, c, h, hid = SHAPE
    buf = encoder_block(np.float32, tokens=t, dim=c, heads=h, hidden=hid, hybrid="asymmetric")
    forms = {}
    for mid, (tag, fused) in enumerate((("fused", True), ("unfused", False))):
        m, ex, key = executor(buf, mid, fused)
        view = ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()
        view[...] = np.random.default_rng(1).normal(0, 1, view.shape)
        for _ in range(3):
            assert ex.ExecuteSubgraph(key).ok()
        forms[tag] = (m, ex, key, ex.GetTensorView(key, ex.GetOutputs(key)[0]).GetData().copy())
        assert np.isfinite(forms[tag][3]).all()
    # the two forms round the LayerNorm's sums in different orders: report how far the block's outputs lie apart
    apart = float(np.abs(forms["fused"][3].astype(np.float64) - forms["unfused"][3].astype(np.float64)).max())
    wall = {tag: [] for tag in forms}
    dev = {tag: [] for tag in forms}
    for _ in range(args.rounds):
        for tag, (m, ex, key, _) in forms.items():
            dev[tag].append(ex.TimeSubgraph(key, iters=200))
            t0 = time.perf_counter()
            for _ in range(args.iters):
                ex.ExecuteSubgraph(key)
            wall[tag].append(1e6 * (time.perf_counter() - t0) / args.iters)
    res = {"model": "encoder_block(float32, %d, %d, %d, %d, hybrid=asymmetric)" % SHAPE, "rounds": args.rounds,
           "iters": args.iters, "lib_variant": os.environ.get("BAND_HIP_LIB_VARIANT", ""),
           "projections_checked_bit_exact": checked, "max_abs_output_difference_between_forms": apart, "forms": {}}
    for tag, (m, ex, key, _) in forms.items():
        rows = ex.ProfileSubgraph(key, iters=20)
        per = {}
        for r in rows:
            k = per.setdefault(r["kernel"], {"launches": 0, "us": 0.0})
            k["launches"] += 1
            k["us"] += 1e3 * r["ms"]
        for k in per.values():
            k["us"] = round(k["us"], 2)
        total = sum(1e3 * r["ms"] for r in rows)
        ln = sum(v["us"] for k, v in per.items() if k in LN_KERNELS)
        res["forms"][tag] = {"launches": len(rows), "kernel_sum_us": round(total, 2),
                             "layernorm_and_quantisation_us": round(ln, 2), "kernels": per,
                             "device_us_per_pass": stats(dev[tag]), "wall_us_per_pass": stats(wall[tag]),
                             "device_us_rounds": [round(v, 2) for v in dev[tag]]}
        print(tag, json.dumps(res["forms"][tag]), flush=True)
    assert res["forms"]["fused"]["launches"] == 20 and "layernorm_f32_kernel" in res["forms"]["fused"]["kernels"]
    assert "layernorm_f32_kernel" not in res["forms"]["unfused"]["kernels"]
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
