#!/usr/bin/env python3
"""The masked attention core (an int8 padding mask ADDed to the scores) as one
launch (BAND_HIP_FUSED_ATTENTION=1) and as the default four launches, beside the
unmasked fused launch of the same shape.

Per shape - a padded encoder_block(196, 192, 3, 768) and padded attention
blocks at (heads, tokens, head dim) = (4, 256, 36) and (12, 64, 64), each with
a second input [1, 1, 1, tokens] (tests.mask_models) - three kGPU executors in
one process: the masked model with the flag, the masked model without it, and
the same block without a mask with the flag.  Alternated over the rounds: the
end-to-end wall time of `iters` ExecuteSubgraph calls (replayed graph) and
TimeSubgraph's device time per pass; once, ProfileSubgraph's per-kernel lines.
Median and min - max over the rounds; the two masked forms' outputs are
compared first.  The default-shape text_encoder with mask=True (an int32 mask
through CAST, SUB, MUL, QUANTIZE, RESHAPE) runs the same way.
Launcher part: what the bias costs inside the launch is bh_attention_i8 with
and without `bias` on ONE operand set per shape (back-to-back launches between
two events on one stream), and cast_kernel (int32 -> float32 at the mask's
shapes) beside bh_copy_d2d of the same output bytes.
Usage: python tools/attn_mask_profile.py [--rounds 7] [--iters 2000] [--out profiles/NAME.json]
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
MASKED, PLAIN = "attention_bias_i8_kernel", "attention_i8_kernel"
CORE = (MASKED, PLAIN, "bmm_mfma_kernel", "softmax_kernel")


def stats(v):
    s = sorted(v)
    return {"median": round(s[len(s) // 2], 2), "min": round(s[0], 2), "max": round(s[-1], 2)}


def launcher_part(args, res):
    import ctypes
    from band_amd import _abi
    from band_amd.device import DeviceBuffer, Stream
    from tests import mask_models as M
    lib = _abi.load()
    st = Stream()
    ev = [ctypes.c_void_p(), ctypes.c_void_p()]
    for e in ev:
        _abi.check(lib.bh_event_create(ctypes.byref(e)), "event")

    def timed(fn):
        for _ in range(10):
            _abi.check(fn(), "launch")
        lib.bh_event_record(ev[0], st.handle)
        for _ in range(args.iters):
            fn()
        lib.bh_event_record(ev[1], st.handle)
        st.sync()
        ms = ctypes.c_float(0)
        _abi.check(lib.bh_event_elapsed_ms(ev[0], ev[1], ctypes.byref(ms)), "elapsed")
        return 1e3 * ms.value / args.iters

    def rounds(variants):
        us = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                us[k].append(timed(fn))
        return {k: {"us_" + n: v for n, v in stats(u).items()} for k, u in us.items()}

    res["launcher"] = {}
    # the scores' quantisation kept by the ADD, a padding bias [b0, 1, 1, keys]: the models' case
    for name, batch, tokens, d in (("heads3_tokens196_dim64", (1, 3), 196, 64), ("heads4_tokens256_dim36", (1, 4), 256, 36),
                                   ("heads12_tokens64_dim64", (1, 12), 64, 64)):
        c = M.BiasCase(name, batch, tokens, tokens, d, d, bias="padding", bias_scale=10000.0 / 255, bias_zp=127,
                       add_scale=0.1, add_zp=7, seed=77)
        c.bias[..., -5:] = -128
        c.bias[..., :-5] = 127
        p, bufs, read = M.prepare(c, True)
        q = _abi.AttentionParams.from_buffer_copy(p)
        q.bias = None
        assert lib.bh_attention_i8_kernel(ctypes.byref(p)) == b"attention_bias_i8_kernel"
        assert lib.bh_attention_i8_kernel(ctypes.byref(q)) == b"attention_i8_kernel"
        _abi.check(lib.bh_attention_i8(ctypes.byref(p), st.handle), "masked")
        st.sync()
        assert np.array_equal(read(), c.ref()), name
        row = rounds({"masked": lambda: lib.bh_attention_i8(ctypes.byref(p), st.handle),
                      "unmasked": lambda: lib.bh_attention_i8(ctypes.byref(q), st.handle)})
        res["launcher"][name] = row
        print(name, json.dumps(row), flush=True)
    for shape in ((1, 128), (32, 128), (1, 196), (32, 512)):
        n = shape[0] * shape[1]
        x = (np.arange(n) % 2).astype(np.int32)
        dx, dy, dz, dsrc = DeviceBuffer.from_array(x), DeviceBuffer(4 * n), DeviceBuffer(4 * n), DeviceBuffer(4 * n)
        cp = _abi.CastParams(_abi.CAST_I32, _abi.CAST_F32, n, dx.value, dy.value)
        _abi.check(lib.bh_cast(ctypes.byref(cp), st.handle), "cast")
        st.sync()
        assert np.array_equal(dy.download(np.float32, (n,)), x.astype(np.float32))
        row = rounds({"cast": lambda: lib.bh_cast(ctypes.byref(cp), st.handle),
                      "copy": lambda: lib.bh_copy_d2d(dz.value, dsrc.value, 4 * n, st.handle)})
        row["bytes_out"] = 4 * n
        res["launcher"]["cast_i32_f32_%dx%d" % shape] = row
        print("cast", shape, json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=2000)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    assert args.rounds >= 7, "at least 7 rounds"
    from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
    from band_amd.tflite_synth import attention_block, encoder_block, text_encoder
    from tests import cast_models as C
    from oracle.tflite_fb import Model as OModel
    from tests import mask_models as M

    shapes = (("encoder_block(196, 192, 3, 768)", lambda: M.padded_encoder(196, 192, 3, 768),
               lambda: encoder_block(np.int8, tokens=196, dim=192, heads=3, hidden=768)),
              ("attention_block(heads 4, tokens 256, head dim 36)", lambda: M.padded_block(256, 144, 4, 1),
               lambda: attention_block(np.int8, tokens=256, dim=144, heads=4)),
              ("attention_block(heads 12, tokens 64, head dim 64)", lambda: M.padded_block(64, 768, 12, 1),
               lambda: attention_block(np.int8, tokens=64, dim=768, heads=12)),
              ("text_encoder(128, 192, 3, 768, 2 blocks, vocab 1000)", lambda: text_encoder(np.int8, mask=True),
               lambda: text_encoder(np.int8)))
    os.environ.pop("BAND_HIP_FUSION", None)
    res = {"rounds": args.rounds, "iters": args.iters, "models": {}}
    mid = 0
    for name, build_masked, build_plain in shapes:
        masked, plain = build_masked(), build_plain()
        forms = {}
        for tag, buf, flag in (("masked_fused", masked, "1"), ("masked_default", masked, None), ("unmasked_fused", plain, "1")):
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
            text = name.startswith("text_encoder")
            feeds = (C.inputs(buf, 0) if buf is masked else {OModel(buf).inputs[0]: C.T.token_ids_any(buf)}) if text \
                else M.model_inputs(buf, seed=0)  # (5 trailing tokens masked)
            for t, v in feeds.items():
                ex.GetTensorView(key, t).GetData()[...] = v
            for _ in range(3):
                assert ex.ExecuteSubgraph(key).ok()
            forms[tag] = (m, ex, key)
            mid += 1
        os.environ.pop(FLAG, None)
        out_t = OModel(masked).outputs[0]
        outs = {t: forms[t][1].GetTensorView(forms[t][2], out_t).GetData().copy() for t in ("masked_fused", "masked_default")}
        assert np.array_equal(outs["masked_fused"], outs["masked_default"]), "the two masked forms differ on " + name
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
            # the core: the fused launch, or the products, the softmax, the head TRANSPOSEs and the ADD on the scores
            core = sum(v["us"] for k, v in per.items() if k in CORE or k.startswith("reindex"))
            if t == "masked_default":
                ops = OModel(masked).operators
                adds = [next(i for i, o in enumerate(ops) if o.outputs[0] == ms)
                        for sc, ms, pr, ctx, bias in M.masked_attention_tensors(masked)]
                core += sum(1e3 * r["ms"] for r in rows if r["op_index"] in adds)
            entry[t] = {"launches": len(rows), "kernel_sum_us": round(sum(1e3 * r["ms"] for r in rows), 2),
                        "attention_core_us": round(core, 2), "kernels": per, "wall_us_per_pass": stats(wall[t]),
                        "device_us_per_pass": stats(dev[t])}
            print(name, t, json.dumps(entry[t]), flush=True)
        assert MASKED in entry["masked_fused"]["kernels"] and MASKED not in entry["masked_default"]["kernels"]
        assert PLAIN in entry["unmasked_fused"]["kernels"]
        res["models"][name] = entry
    launcher_part(args, res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
