#!/usr/bin/env python3
"""Device time of bh_gather beside bh_copy_d2d of the same output bytes, and
text_encoder on a kGPU executor.

Launcher part, per embedding shape ([30522, 128], [30522, 768], [1000, 192];
int8 and float32; 128 ids, and 128 x 32 for the job-batched pass):
  gather   bh_gather of random in-range ids (gather_rows_kernel)
  copy     bh_copy_d2d of the output's byte count, the floor for a copy
alternated inside one process: per round each variant is `iters` launches back
to back on one stream between two events; the figure is the mean per launch,
so it holds one dispatch (the ~empty-launch floor) and the kernel.  Median and
min - max over the rounds.

Model part, text_encoder() at its default shape, int8 and hybrid, with the
default launches and under each opt-in fusion flag that applies:
  us_per_pass        TimeSubgraph (device, passes back to back, graph replay)
  launches           per pass
  gather_us / share  the GATHER launch's own duration (ProfileSubgraph) and its
                     share of the sum over the pass's launches
at batch 1 and for 8 jobs in one pass (the model built at batch 8: the launches
of the job-batch variant); job_batch_8_host_us is a host clock around
ExecuteJobBatch(key, 8), transfers and synchronisation included.
Usage: python tools/gather_profile.py [--rounds 7] [--iters 200] [--out profiles/NAME.json]
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

TABLES = [(30522, 128), (30522, 768), (1000, 192)]
FLAGS = {"int8": (None, "BAND_HIP_FUSED_ATTENTION"), "hybrid": (None, "BAND_HIP_FUSED_LAYERNORM_F32")}


def launcher_part(args, res):
    from band_amd import _abi
    from band_amd.device import DeviceBuffer, Stream
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

    rng = np.random.default_rng(0)
    for vocab, dim in TABLES:
        for dtype in (np.int8, np.float32):
            table = rng.integers(-100, 100, (vocab, dim)).astype(dtype)
            dt = DeviceBuffer.from_array(table)
            for n_idx in (128, 128 * 32):
                name = "%dx%d_%s_ids%d" % (vocab, dim, np.dtype(dtype).name, n_idx)
                ids = rng.integers(0, vocab, n_idx).astype(np.int32)
                want = table[ids]
                di = DeviceBuffer.from_array(ids)
                dy, dz, dsrc = DeviceBuffer(want.nbytes), DeviceBuffer(want.nbytes), DeviceBuffer(want.nbytes)
                p = _abi.GatherParams(elem_bytes=table.itemsize, index_bytes=4, outer=1, axis_size=vocab, n_idx=n_idx,
                                      inner=dim, params=dt.value, indices=di.value, output=dy.value)
                variants = {"gather": lambda: lib.bh_gather(ctypes.byref(p), st.handle),
                            "copy": lambda: lib.bh_copy_d2d(dz.value, dsrc.value, want.nbytes, st.handle)}
                _abi.check(variants["gather"](), "gather")  # right before it is timed
                st.sync()
                assert np.array_equal(dy.download(dtype, want.shape), want), name
                us = {k: [] for k in variants}
                for _ in range(args.rounds):
                    for k, fn in variants.items():
                        us[k].append(timed(fn))
                row = {"kernel": lib.bh_gather_kernel(ctypes.byref(p)).decode(), "bytes_out": int(want.nbytes)}
                for k, v in us.items():
                    s = sorted(v)
                    row[k] = {"us_median": round(s[len(s) // 2], 2), "us_min": round(s[0], 2), "us_max": round(s[-1], 2)}
                res["launcher"][name] = row
                print(name, json.dumps(row), flush=True)
                for b in (di, dy, dz, dsrc):
                    b.free()
            dt.free()


def model_part(args, res):
    from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
    from band_amd.tflite_synth import text_encoder
    rng = np.random.default_rng(1)
    mid = 0
    for form, flags in FLAGS.items():
        kw = dict(dtype=np.int8) if form == "int8" else dict(dtype=np.float32, hybrid="symmetric")
        for flag in flags:
            for f in ("BAND_HIP_FUSED_ATTENTION", "BAND_HIP_FUSED_LAYERNORM_F32"):
                os.environ.pop(f, None)
            if flag:
                os.environ[flag] = "1"
            row = {}
            for batch in (1, 8):
                mid += 1
                m = HipModel(mid)
                assert m.FromBuffer(text_encoder(batch=batch, **kw)).ok()
                ex = HipModelExecutor(mid, 1, DeviceFlag.kGPU)
                st = ex.PrepareSubgraph(m)
                assert st.ok(), st.message()
                key = SubgraphKey(mid, 1)
                t_in = ex.GetInputs(key)[0]
                ex.GetTensorView(key, t_in).GetData()[...] = rng.integers(0, 1000, (batch, 128)).astype(np.int32)
                for _ in range(3):
                    assert ex.ExecuteSubgraph(key).ok()
                us = sorted(ex.TimeSubgraph(key, args.iters) for _ in range(args.rounds))
                prof = ex.ProfileSubgraph(key, iters=20)
                total = sum(r["ms"] for r in prof)
                gather = [r["ms"] for r in prof if r["kernel"] == "gather_rows_kernel"]
                assert len(gather) == 1
                row["batch_%d" % batch] = {"us_per_pass": round(us[len(us) // 2], 1), "us_min": round(us[0], 1),
                                           "us_max": round(us[-1], 1), "launches": len(prof),
                                           "gather_us": round(1e3 * gather[0], 2),
                                           "gather_share_of_kernel_time": round(gather[0] / total, 4)}
                if batch == 1:
                    assert ex.PrepareJobBatches(m, key, 8).ok()
                    for s in range(8):
                        ex.GetJobSlotView(key, t_in, 8, s).GetData()[...] = rng.integers(0, 1000, (1, 128)).astype(np.int32)
                    for _ in range(3):
                        assert ex.ExecuteJobBatch(key, 8).ok()
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        ex.ExecuteJobBatch(key, 8)
                    row["job_batch_8_host_us"] = round(1e6 * (time.perf_counter() - t0) / args.iters, 1)
                    row["job_batch_8_launches"] = len(ex.JobBatchLaunchKernels(key, 8))
                    t0 = time.perf_counter()
                    for _ in range(args.iters):
                        ex.ExecuteSubgraph(key)
                    row["batch_1_host_us"] = round(1e6 * (time.perf_counter() - t0) / args.iters, 1)
                del ex
            name = "text_encoder_%s%s" % (form, "_" + flag.lower() if flag else "")
            res["models"][name] = row
            print(name, json.dumps(row), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--out", default="")
    ap.add_argument("--skip-models", action="store_true")
    args = ap.parse_args()
    res = {"rounds": args.rounds, "iters": args.iters, "launcher": {}, "models": {}}
    launcher_part(args, res)
    if not args.skip_models:
        model_part(args, res)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
