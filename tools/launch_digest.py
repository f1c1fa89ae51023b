#!/usr/bin/env python3
"""The prepared launch list of a fixed set of models, as text to diff.

For every model the whole-model subgraph is prepared (of a model the worker
splits, the worker's ops as one subgraph) and one line per launch is made:
the launch's position, the kernel symbol (LaunchKernels) and, on a device, the
op index, alg_ops and alg_bytes (ProfileSubgraph(iters=1)).  --full prints
those lines; the default prints one line per model, with their SHA-256 and the
count of each kernel, which is what is kept under profiles/.  Two builds of
the library that lower a model alike print the same bytes, so a refactor of
the lowering is checked with

    python tools/launch_digest.py --device cpu > a.txt      (on each build)

Models: the synthesiser's MobileNetV2 / V1, ShuffleNet, attention block,
ViT-tiny (bare, and with LayerNorm and MLP), encoder block, SSD (with and
without postprocess), EfficientDet-Lite2 at 448, DeepLab (with argmax) and
PoseNet, int8 and uint8 where the synthesiser builds both; from the tests'
builders the float32 encoder block with hybrid FULLY_CONNECTEDs and a
MobileNetV2 of hybrid convs; and every .tflite under tests/golden/.  The
opt-in launches show when the run sets their variables (BAND_HIP_FUSED_ATTENTION,
BAND_HIP_FUSED_LAYERNORM_F32, BAND_HIP_HYBRID_CONV, BAND_HIP_GPU_DETECTION).

Job batches: PrepareJobBatches(max_batch=4) is run on every model and its
status printed, so a variant that no longer lowers shows.  The variants'
own launch lists are not reachable through the Python API; what is printed
per batch 2..4 is the launch list of the synthesiser's batch-B build of the
model, which is the model a variant executor lowers (HipModel::CloneWithJobBatch
scales axis 0 of every non-constant tensor).  The golden files get the status
line only.

On a device run with BAND_HIP_AUTOTUNE=0: the static model, not a timing,
then picks the fused forms.
Usage: python tools/launch_digest.py [--device cpu|gpu] [--models NAME,...] [--full]
"""
import argparse
import collections
import glob
import hashlib
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def synth_models():
    """name -> build(batch) of every synthesised model"""
    from band_amd import tflite_synth as S
    both = {
        "mobilenet_v2": S.mobilenet_v2, "mobilenet_v1": S.mobilenet_v1, "shufflenet_v1": S.shufflenet_v1,
        "ssd_mobilenet_v2": S.ssd_mobilenet_v2,
        "ssd_mobilenet_v2_post": lambda dt, batch: S.ssd_mobilenet_v2(dt, batch=batch, postprocess=True),
        "efficientdet_lite2_448": lambda dt, batch: S.efficientdet_lite2(dt, size=448, batch=batch),
        "deeplab_v3": S.deeplab_v3_mobilenet_v2,
        "deeplab_v3_argmax": lambda dt, batch: S.deeplab_v3_mobilenet_v2(dt, batch=batch, argmax=np.int32),
        "posenet": S.posenet_mobilenet_v1,
    }
    out = {}
    for name, fn in both.items():
        for dt in (np.int8, np.uint8):
            out["%s_%s" % (name, np.dtype(dt).name)] = (lambda fn, dt: lambda batch: fn(dt, batch=batch))(fn, dt)
    out["attention_block_int8"] = lambda batch: S.attention_block(np.int8, batch=batch)  # BATCH_MATMUL: int8 only
    out["vit_tiny_int8"] = lambda batch: S.vit_tiny(np.int8, batch=batch)
    out["encoder_block_int8"] = lambda batch: S.encoder_block(np.int8, batch=batch)  # int8 LayerNorm + GELU
    out["vit_tiny_ln_mlp_int8"] = lambda batch: S.vit_tiny(np.int8, batch=batch, layer_norm=True, mlp=True)
    return out


def test_models():
    """name -> build() of the models taken from the tests' builders (batch 1 only)"""
    from tests import hybrid_conv_models, layernorm_f32_models
    return {
        # float32 encoder block, hybrid FULLY_CONNECTED, Q / K / V as extra outputs (float32 LayerNorm)
        "encoder_f32_hybrid_qkv": lambda: layernorm_f32_models.encoder_with_qkv_outputs("symmetric"),
        # MobileNetV2 at 32 x 32 with every conv hybrid
        "mobilenet_v2_32_hybrid_conv": hybrid_conv_models.MODELS["mobilenet_v2_32_all"],
    }


def digest(name, buf, device, mid, batches, full):
    from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
    gpu = device == "gpu"
    worker = 1 if gpu else 0
    m = HipModel(mid)
    if not m.FromBuffer(buf).ok():
        print("%s: cannot load" % name)
        return
    flag = DeviceFlag.kGPU if gpu else DeviceFlag.kCPU
    ex = HipModelExecutor(mid, worker, flag)
    spec = ex.InvestigateModelSpec(m)
    ops = [i for i in range(spec.num_ops) if i not in spec.unsupported_ops[flag]]
    if len(ops) < spec.num_ops:  # a split model: the worker's part as one subgraph, as bench.py profiles it
        print("%s: ops not in the worker's set: %s" % (name, sorted(spec.unsupported_ops[flag])))
    st = ex.PrepareSubgraph(m, ops if len(ops) < spec.num_ops else ())
    if not st.ok():
        print("%s: PrepareSubgraph: %s" % (name, st.message()))
        return
    key = SubgraphKey(mid, worker)
    kernels = ex.LaunchKernels(key)
    rows = ex.ProfileSubgraph(key, iters=1) if gpu else None
    lines = []
    for i, k in enumerate(kernels):
        if rows:
            assert rows[i]["kernel"] == k
            lines.append("  %3d op %3d %-44s ops %.17g bytes %.17g" % (i, rows[i]["op_index"], k, rows[i]["alg_ops"],
                                                                     rows[i]["alg_bytes"]))
        else:
            lines.append("  %3d %s" % (i, k))
    if full:
        print("%s: %d launches" % (name, len(kernels)))
        print("\n".join(lines))
    else:  # one line: the launch lines' hash and how often each kernel occurs
        count = collections.Counter(kernels)
        print("%s: %d launches, sha256 %s: %s" % (
            name, len(kernels), hashlib.sha256("\n".join(lines).encode()).hexdigest()[:32],
            ", ".join("%d %s" % (n, k) for k, n in sorted(count.items()))))
    if batches:
        st = ex.PrepareJobBatches(m, key, 4)
        print("%s: PrepareJobBatches(4): %s, max job batch %d" % (name, "ok" if st.ok() else st.message(),
                                                                   ex.MaxJobBatch(key)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", choices=("cpu", "gpu"), default="cpu")
    ap.add_argument("--models", default="")
    ap.add_argument("--full", action="store_true", help="one line per launch instead of one per model")
    a = ap.parse_args()
    if a.device == "gpu":
        from band_amd import SetWorkerDevice
        SetWorkerDevice(1, 0)
    want = set(a.models.split(",")) if a.models else None
    mid = 0
    for name, build in synth_models().items():
        if want and name not in want:
            continue
        digest(name, build(1), a.device, mid, True, a.full)
        mid += 1
        for b in (2, 3, 4):
            digest("%s batch %d" % (name, b), build(b), a.device, mid, False, a.full)
            mid += 1
    for name, build in test_models().items():
        if want and name not in want:
            continue
        digest(name, build(), a.device, mid, True, a.full)
        mid += 1
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "golden", "*.tflite"))):
        name = os.path.basename(path)
        if want and name not in want:
            continue
        with open(path, "rb") as f:
            digest(name, f.read(), a.device, mid, True, a.full)
        mid += 1


if __name__ == "__main__":
    main()
