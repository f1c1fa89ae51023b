#!/usr/bin/env python3
"""Device time of the re-indexing kernels beside bh_copy_d2d of the same bytes.

Per shape (the zoo's maps at batch 1 and 32, the launcher cases' transposes):
  routed   bh_reindex, the form the launcher picks (named in the output)
  gather   bh_reindex_as(gather=1): reindex_gather_kernel on the same map
  copy     bh_copy_d2d of the output's byte count, the floor for a copy
alternated inside one process: per round each variant is `iters` launches back
to back on one stream between two events; the figure is the mean per launch,
so it holds one dispatch (the ~empty-launch floor) and the kernel.  Median and
min - max over the rounds, and GB/s as 2 x output bytes / time.
Usage: python tools/reindex_profile.py [--rounds 7] [--iters 200] [--out profiles/NAME.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def shapes():
    """[(name, dtype, input shape, view)]"""
    out = []
    for b in (1, 32):
        out += [
            ("split_channels_32to16_b%d" % b, np.int8, (b, 14, 14, 32), lambda x: x[..., 16:]),
            ("space_to_depth_16x16x3_b%d" % b, np.int8, (b, 16, 16, 3),
             lambda x: x.reshape(x.shape[0], 8, 2, 8, 2, 3).transpose(0, 1, 3, 2, 4, 5)),
            ("depth_to_space_8x8x12_b%d" % b, np.int8, (b, 8, 8, 12),
             lambda x: x.reshape(x.shape[0], 8, 8, 2, 2, 3).transpose(0, 1, 3, 2, 4, 5)),
            ("head_transpose_7x7x3x9_b%d" % b, np.int8, (b, 7, 7, 3, 9), lambda x: x.transpose(0, 3, 1, 2, 4)),
            ("shuffle_14x14x2x16_b%d" % b, np.int8, (b, 14, 14, 2, 16), lambda x: x.transpose(0, 1, 2, 4, 3)),
            ("nhwc_to_nchw_64x64x16_b%d" % b, np.int8, (b, 64, 64, 16), lambda x: x.transpose(0, 3, 1, 2)),
            ("nchw_to_nhwc_16x64x64_b%d" % b, np.int8, (b, 16, 64, 64), lambda x: x.transpose(0, 2, 3, 1)),
            ("nhwc_to_nchw_64x64x16_f32_b%d" % b, np.float32, (b, 64, 64, 16), lambda x: x.transpose(0, 3, 1, 2)),
            ("nhwc_to_nchw_224x224x3_b%d" % b, np.int8, (b, 224, 224, 3), lambda x: x.transpose(0, 3, 1, 2)),
            ("reverse_channels_14x14x32_b%d" % b, np.int8, (b, 14, 14, 32), lambda x: x[..., ::-1]),
            ("head_objectness_3x7x7x9_b%d" % b, np.int8, (b, 3, 7, 7, 9), lambda x: x[..., 4:5]),
        ]
    out += [
        ("transpose_1024x1024_i8", np.int8, (1024, 1024), lambda x: x.T),
        ("transpose_1024x1024_f32", np.float32, (1024, 1024), lambda x: x.T),
        ("transpose_4096x4096_i8", np.int8, (4096, 4096), lambda x: x.T),
        ("transpose_4096x4096_f32", np.float32, (4096, 4096), lambda x: x.T),
        ("nhwc_to_nchw_112x112x64_b32", np.int8, (32, 112, 112, 64), lambda x: x.transpose(0, 3, 1, 2)),
        ("nchw_to_nhwc_64x112x112_b32", np.int8, (32, 64, 112, 112), lambda x: x.transpose(0, 2, 3, 1)),
    ]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default="")
    ap.add_argument("--only", default="", help="substring a shape's name must contain")
    args = ap.parse_args()
    from band_amd import _abi
    from band_amd.device import DeviceBuffer, Stream
    from tests.reindex_models import fill, reindex_params
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

    res = {"rounds": args.rounds, "iters": args.iters, "shapes": {}}
    for name, dtype, shape, view in shapes():
        if args.only not in name:
            continue
        x = fill(shape, dtype)
        v = view(x)
        want = np.ascontiguousarray(v)
        dx, dy, dz = DeviceBuffer.from_array(x), DeviceBuffer(want.nbytes), DeviceBuffer(want.nbytes)
        p = reindex_params(x, v, dx.value, dy.value)
        variants = {"routed": lambda: lib.bh_reindex(ctypes.byref(p), st.handle),
                    "gather": lambda: lib.bh_reindex_as(ctypes.byref(p), 1, st.handle),
                    "copy": lambda: lib.bh_copy_d2d(dz.value, dx.value, want.nbytes, st.handle)}
        for k in ("routed", "gather"):  # both forms are right before either is timed
            dy.upload(np.zeros(want.nbytes, np.uint8))
            _abi.check(variants[k](), k)
            st.sync()
            assert np.array_equal(dy.download(dtype, want.shape), want), (name, k)
        us = {k: [] for k in variants}
        for _ in range(args.rounds):
            for k, fn in variants.items():
                us[k].append(timed(fn))
        row = {"kernel": lib.bh_reindex_kernel(ctypes.byref(p)).decode(), "bytes_out": int(want.nbytes)}
        for k, v_ in us.items():
            s = sorted(v_)
            med = s[len(s) // 2]
            row[k] = {"us_median": round(med, 2), "us_min": round(s[0], 2), "us_max": round(s[-1], 2),
                      "gbps": round(2 * want.nbytes / med / 1e3, 1)}
        res["shapes"][name] = row
        print(name, json.dumps(row), flush=True)
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
