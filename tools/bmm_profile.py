#!/usr/bin/env python3
"""Device time of bh_batch_matmul_i8 on attention shapes, beside its yardsticks.

Per (heads, tokens, head dim) and job batch, for Q K^T (adj_y: both operands
K-contiguous, read straight from global memory) and P V (rhs K-strided, staged
transposed through LDS):
  routed   bh_batch_matmul_i8 as the launcher routes it
  nt1, nt4 one and four 16-column tiles per wave, pinned (BH_BMM_NT1 / BH_BMM_NT4)
  byte_units  the routed form with 1-byte fragment units (BH_BMM_BYTES)
  conv1x1  bh_conv2d_i8 on the same number of rows, K and N as ONE 1x1 conv
           whose filter is the first rhs slice pre-packed as a constant: the
           same MACs and lhs / output bytes with prepare-time packing - what an
           activation-operand kernel can approach but need not beat
  copy     bh_copy_d2d of operands + output bytes, the dispatch floor
alternated inside one process: per round each variant is `iters` launches back
to back on one stream between two events; the figure is the mean per launch.
Median and min - max over the rounds.  The P V rows also time the three
transposed reads of the staged rhs, pinned (BH_BMM_READ_*): read_b128
(byte-transposing LDS writes + ds_read_b128), read_gather (row-major image,
16 byte reads), read_tr8 (row-major image, two ds_read_b64_tr_b8).
Usage: python tools/bmm_profile.py [--rounds 5] [--iters 200] [--out profiles/NAME.json]
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [(3, 196, 64), (4, 256, 36), (12, 64, 64)]
JOB_BATCHES = (1, 24)


def conv1x1_params(lib, keep, rows, K, N, x_ptr, w_nk, zps, mult, shift, out_ptr):
    """bh_conv_params of [1, rows, 1, K] x filter [N, 1, 1, K] with the product's quantisation"""
    from band_amd import _abi
    from band_amd.device import DeviceBuffer
    z_l, z_r, z_o = zps
    kp, npd = ctypes.c_int(), ctypes.c_int()
    _abi.check(lib.bh_conv_packed_geometry(N, K, ctypes.byref(kp), ctypes.byref(npd)), "geom")
    packed = np.zeros((npd.value, kp.value), np.int8)
    beff = np.zeros(N, np.int32)
    w = np.ascontiguousarray(w_nk.astype(np.int16) - z_r).clip(-128, 127).astype(np.int8)  # symmetric filter
    bias = np.zeros(N, np.int32)
    _abi.check(lib.bh_pack_conv_weights(w.ctypes.data_as(ctypes.c_void_p), 1, N, K, kp.value, npd.value,
                                        bias.ctypes.data_as(ctypes.c_void_p), z_l, 0,
                                        packed.ctypes.data_as(ctypes.c_void_p), beff.ctypes.data_as(ctypes.c_void_p)), "pack")
    m32, s32 = np.full(N, mult, np.int32), np.full(N, shift, np.int32)
    bufs = [DeviceBuffer.from_array(a) for a in (packed, beff, m32, s32)]
    keep += bufs
    q = _abi.ConvParams()
    q.batch, q.in_h, q.in_w, q.in_c = 1, rows, 1, K
    q.out_h, q.out_w, q.out_c = rows, 1, N
    q.k_h = q.k_w = q.stride_h = q.stride_w = q.dil_h = q.dil_w = 1
    q.k_pad, q.n_pad = kp.value, npd.value
    q.in_zp, q.w_zp, q.out_zp, q.act_min, q.act_max = z_l, 0, z_o, -128, 127
    q.input, q.output = x_ptr, out_ptr
    q.weights, q.bias_eff, q.mult, q.shift = (b.value for b in bufs)
    q.requant_fast = lib.bh_conv_requant_fast_ok(m32.ctypes.data_as(ctypes.c_void_p), s32.ctypes.data_as(ctypes.c_void_p),
                                                 N, K, 0)
    return q


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default="")
    args = ap.parse_args()
    from band_amd import _abi
    from band_amd.device import DeviceBuffer, Stream
    from tests import bmm_models as B
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
    for H, T, D in SHAPES:
        for jb in JOB_BATCHES:
            for kind in ("qk", "pv"):
                if kind == "qk":   # [jb, H, T, D] x [jb, H, T, D]^T, operands ~45 LSBs around their zero points
                    case = B.BmmCase("qk", (jb, H, T, D), (jb, H, T, D), adj_y=True, zps=(3, -5, 7), spread=45,
                                     scales=(0.05, 0.05, 0.05 * 0.05 * np.sqrt(D) * 45 * 45 / 32), seed=1)
                else:              # softmax output (zero point -128, scale 1 / 256) x [jb, H, T, D]
                    case = B.BmmCase("pv", (jb, H, T, T), (jb, H, T, D), zps=(-128, 4, -6), spread=45,
                                     scales=(1.0 / 256, 0.05, 0.05), seed=2)
                    case.lhs = np.clip(np.random.default_rng(3).exponential(256.0 / T, case.lhs.shape) - 128, -128,
                                       127).astype(np.int8)
                m, n, k = case.mnk
                name = "%s_h%d_t%d_d%d_b%d" % (kind, H, T, D, jb)
                want = B.bmm_ref(case)
                dl, dr = DeviceBuffer.from_array(case.lhs), DeviceBuffer.from_array(case.rhs)
                dy, dz = DeviceBuffer(want.nbytes), DeviceBuffer(case.lhs.nbytes + case.rhs.nbytes + want.nbytes)
                dsrc = DeviceBuffer(case.lhs.nbytes + case.rhs.nbytes + want.nbytes)
                p = B.bmm_params(case, dl.value, dr.value, dy.value)
                pb = B.bmm_params(case, dl.value, dr.value, dy.value)
                pb.kernel_hint = _abi.BMM_BYTES
                p1 = B.bmm_params(case, dl.value, dr.value, dy.value)
                p1.kernel_hint = _abi.BMM_NT1
                p4 = B.bmm_params(case, dl.value, dr.value, dy.value)
                p4.kernel_hint = _abi.BMM_NT4
                reads = {}
                if kind == "pv":  # the staged rhs: its three transposed reads, pinned
                    for tag, bit in (("read_b128", _abi.BMM_READ_B128), ("read_gather", _abi.BMM_READ_GATHER),
                                     ("read_tr8", _abi.BMM_READ_TR8)):
                        reads[tag] = B.bmm_params(case, dl.value, dr.value, dy.value)
                        reads[tag].kernel_hint = bit
                keep = []
                rows = jb * H * m
                w_nk = case.views()[1][0, 0].T
                q = conv1x1_params(lib, keep, rows, k, n, dl.value, w_nk, (case.z_l, case.z_r, case.z_o), case.mult,
                                   case.shift, dy.value)
                total = case.lhs.nbytes + case.rhs.nbytes + want.nbytes
                variants = {"routed": lambda: lib.bh_batch_matmul_i8(ctypes.byref(p), st.handle),
                            "nt1": lambda: lib.bh_batch_matmul_i8(ctypes.byref(p1), st.handle),
                            "nt4": lambda: lib.bh_batch_matmul_i8(ctypes.byref(p4), st.handle),
                            "byte_units": lambda: lib.bh_batch_matmul_i8(ctypes.byref(pb), st.handle),
                            "conv1x1": lambda: lib.bh_conv2d_i8(ctypes.byref(q), st.handle),
                            "copy": lambda: lib.bh_copy_d2d(dz.value, dsrc.value, total, st.handle)}
                for tag, pr in reads.items():
                    variants[tag] = lambda pr=pr: lib.bh_batch_matmul_i8(ctypes.byref(pr), st.handle)
                for v in ["routed", "nt1", "nt4", "byte_units"] + list(reads):  # all are right before any is timed
                    dy.upload(np.zeros(want.nbytes, np.uint8))
                    _abi.check(variants[v](), v)
                    st.sync()
                    assert np.array_equal(dy.download(np.int8, want.shape), want), (name, v)
                us = {v: [] for v in variants}
                for _ in range(args.rounds):
                    for v, fn in variants.items():
                        us[v].append(timed(fn))
                row = {"m": m, "n": n, "k": k, "matrices": jb * H, "bytes": int(total),
                       "conv_kernel": lib.bh_conv2d_i8_kernel(ctypes.byref(q)).decode()}
                for v, t in us.items():
                    s = sorted(t)
                    med = s[len(s) // 2]
                    row[v] = {"us_median": round(med, 2), "us_min": round(s[0], 2), "us_max": round(s[-1], 2)}
                row["routed"]["tops"] = round(2.0 * jb * H * m * n * k / row["routed"]["us_median"] / 1e6, 2)
                res["shapes"][name] = row
                print(name, json.dumps(row), flush=True)
    text = json.dumps(res, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
