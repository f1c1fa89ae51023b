#!/usr/bin/env python3
"""Device time of DeepLab with the segmentation map computed on the device.

Variants, alternated inside one process at every batch (--batches):
  logits    the model as bench.py runs it (argmax=None): 21 bytes per pixel out
  two       the ARG_MAX model lowered as RESIZE_BILINEAR + ARG_MAX launches
            (BAND_HIP_FUSION=noargmax)
  folded    the ARG_MAX model with the fused resize_bilinear_argminmax_kernel
and, with --baseline VARIANT, the logits model on another build of the
library (band_amd/libband_hip_VARIANT.so, e.g. the parent commit's), run in a
child process before and after the alternated rounds.

Per variant and batch: graph-replay time per pass with its host copies
(TimeSubgraph; every round's figure, so the spread shows), the kernel-only
sum and the resize / argminmax / folded kernels' own durations
(ProfileSubgraph), and the device-to-host bytes per job from the output
shapes.  Writes one JSON (--out) and prints it.
Usage: python tools/argmax_profile.py [--size 224] [--batches 1,32] [--rounds 5]
       [--iters 100] [--baseline parent] [--out profiles/NAME.json]
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

TAIL_KERNELS = ("resize_bilinear_kernel", "argminmax_kernel", "argminmax_row_kernel",
                "resize_bilinear_argminmax_kernel")


def make_executor(buf, mid, fusion):
    """an executor of model bytes `buf` on GPU worker 1, bound under BAND_HIP_FUSION=fusion"""
    from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
    old = os.environ.pop("BAND_HIP_FUSION", None)
    if fusion:
        os.environ["BAND_HIP_FUSION"] = fusion
    try:
        m = HipModel(mid)
        assert m.FromBuffer(buf).ok()
        ex = HipModelExecutor(mid, 1, DeviceFlag.kGPU)
        st = ex.PrepareSubgraph(m)
        assert st.ok(), st.message()
    finally:
        os.environ.pop("BAND_HIP_FUSION", None)
        if old is not None:
            os.environ["BAND_HIP_FUSION"] = old
    ex._model_ref = m
    key = SubgraphKey(mid, 1)
    shape = ex.GetTensorView(key, ex.GetInputs(key)[0]).GetDims()
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = np.random.default_rng(0).integers(
        -128, 128, shape).astype(np.int8)
    for _ in range(3):
        assert ex.ExecuteSubgraph(key).ok()
    return ex, key


def measure(variants, batch, rounds, iters):
    """variants: {name: (executor, key)}; alternates TimeSubgraph over them"""
    out = {name: {"replay_us_rounds": []} for name in variants}
    for name, (ex, key) in variants.items():
        ex.TimeSubgraph(key, iters=20)
    for _ in range(rounds):
        for name, (ex, key) in variants.items():
            out[name]["replay_us_rounds"].append(round(ex.TimeSubgraph(key, iters=iters), 2))
    for name, (ex, key) in variants.items():
        r = sorted(out[name]["replay_us_rounds"])
        rows = ex.ProfileSubgraph(key, iters=20)
        d2h = sum(ex.GetTensorView(key, t).GetBytes() for t in ex.GetOutputs(key))
        out[name].update(replay_us_median=r[len(r) // 2], replay_us_min=r[0], replay_us_max=r[-1],
                         kernel_sum_us=round(sum(x["ms"] for x in rows) * 1e3, 2), launches=len(rows),
                         # the model's last launches (the ASPP's small resize comes earlier)
                         tail_kernels_us={x["kernel"]: round(x["ms"] * 1e3, 2) for x in rows[-2:]
                                          if x["kernel"] in TAIL_KERNELS},
                         d2h_bytes_per_job=d2h // batch)
    return out


def run(args, only_logits):
    import band_amd
    from band_amd import _abi, tflite_synth as S
    if only_logits:  # another build of the library: it may lack this tree's newest launchers
        for sym in ("bh_argminmax", "bh_argminmax_kernel", "bh_resize_bilinear_argminmax_i8",
                    "bh_resize_bilinear_argminmax_i8_ok"):
            _abi.KERNEL_SYMBOLS.pop(sym, None)
    band_amd.SetWorkerDevice(1, 0)
    res = {}
    for b in args.batches:
        variants = {"logits": make_executor(S.deeplab_v3_mobilenet_v2(np.int8, size=args.size, batch=b), 10, None)}
        if not only_logits:
            am = S.deeplab_v3_mobilenet_v2(np.int8, size=args.size, batch=b, argmax=np.int32)
            variants["two"] = make_executor(am, 11, "noargmax")
            variants["folded"] = make_executor(am, 12, None)
        res["batch_%d" % b] = measure(variants, b, args.rounds, args.iters)
        del variants
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--batches", type=lambda s: [int(v) for v in s.split(",")], default=[1, 32])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=100)
    ap.add_argument("--baseline", default="", help="library variant of the baseline (libband_hip_<name>.so)")
    ap.add_argument("--out", default="")
    ap.add_argument("--only-logits", action="store_true", help="(the baseline child) the logits model alone")
    args = ap.parse_args()
    if args.only_logits:
        print("RESULT " + json.dumps(run(args, True)), flush=True)
        return

    def baseline():
        env = dict(os.environ, BAND_HIP_LIB_VARIANT=args.baseline)
        cmd = [sys.executable, os.path.abspath(__file__), "--only-logits", "--size", str(args.size), "--batches",
               ",".join(str(b) for b in args.batches), "--rounds", str(args.rounds), "--iters", str(args.iters)]
        r = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
        lines = [ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")]
        if r.returncode != 0 or not lines:
            return {"error": (r.stderr or r.stdout)[-400:]}
        return json.loads(lines[-1][7:])

    out = {"model": "deeplab_v3_mobilenet_v2 int8", "size": args.size, "rounds": args.rounds, "iters": args.iters}
    if args.baseline:
        out["baseline_before"] = baseline()
    out["this_tree"] = run(args, False)
    if args.baseline:
        out["baseline_after"] = baseline()
        out["baseline_library"] = "libband_hip_%s.so" % args.baseline
    text = json.dumps(out, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(text, flush=True)


if __name__ == "__main__":
    main()
