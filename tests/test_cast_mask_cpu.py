"""CAST and the padded text models without a GPU: CpuCast over all 16 type pairs
(NaN, +-inf, +-2^31, +-2^63 and -0.5 among the values) against
tests.cast_models.cast_ref, one-op CAST models on the kCPU executor, the
refusals with their reasons, text_encoder(mask=True, pooler=True,
embedding_lookup=True) as int8 / float32 / hybrid on the kCPU executor with
every tensor viewed (5 and 0 masked tokens in the two batch items), job batches
2 and 3, the exact masked-ids test on the float32 model, and CpuCast / CastArgs
under AddressSanitizer / UBSan as a stand-alone program."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi
from oracle.tflite_fb import Model as OModel
from tests import cast_models as C
from tests.graph_reference import run_reference
from tests.test_float_cpu import assert_float_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PAIRS = [(a, b) for a in C.TYPES for b in C.TYPES]
PAIR_IDS = ["%s_to_%s" % (np.dtype(a).name, np.dtype(b).name) for a, b in PAIRS]


def _model(buf, mid=0):
    from band_amd import backend  # noqa: F401
    m = HipModel(mid)
    st = m.FromBuffer(buf)
    assert st.ok(), st.message()
    return m


def test_reference_rule_on_the_named_values():
    """the rule itself, on the reference alone"""
    x = np.array([np.nan, np.inf, -np.inf, 2.0 ** 31, -2.0 ** 31, 2.0 ** 63, -2.0 ** 63, -0.5, 255.9, 256.0, -1.0], np.float32)
    np.testing.assert_array_equal(C.cast_ref(x, np.int32), [0, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 2 ** 31 - 1, -2 ** 31, 0,
                                                            255, 256, -1])
    np.testing.assert_array_equal(C.cast_ref(x, np.int64), [0, 2 ** 63 - 1, -2 ** 63, 2 ** 31, -2 ** 31, 2 ** 63 - 1, -2 ** 63, 0,
                                                            255, 256, -1])
    np.testing.assert_array_equal(C.cast_ref(x, np.uint8), [0, 255, 0, 255, 0, 255, 0, 0, 255, 255, 0])
    inside = np.array([3.7, -3.7, 100.0, 0.0], np.float32)
    np.testing.assert_array_equal(C.cast_ref(inside, np.int32), inside.astype(np.int32))


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_cpu_cast_every_pair(pair):
    from band_amd import backend  # noqa: F401
    lib = _abi.load()
    src_t, dst_t = pair
    for count in C.COUNTS:
        for off in (0, 1):  # the twin takes any alignment
            x = C.source(src_t, count)
            raw = np.concatenate([np.zeros(off, np.uint8), x.view(np.uint8)])
            want = C.cast_ref(x, dst_t)
            out = np.full(off + want.nbytes + 16, 0xff, np.uint8)
            p = _abi.CastParams(C.CODE[np.dtype(src_t)], C.CODE[np.dtype(dst_t)], count, raw.ctypes.data + off,
                                out.ctypes.data + off)
            assert lib.bhx_cpu_cast(ctypes.byref(p)) == 0, lib.bhx_last_error()
            got = out[off:off + want.nbytes].copy().view(dst_t)
            assert got.tobytes() == want.tobytes(), (count, off, x[got != want][:5], got[got != want][:5], want[got != want][:5])
            assert (out[:off] == 0xff).all() and (out[off + want.nbytes:] == 0xff).all()
    p.in_type = 5
    assert lib.bhx_cpu_cast(ctypes.byref(p)) != 0


@pytest.mark.parametrize("pair", PAIRS, ids=PAIR_IDS)
def test_one_cast_models(pair):
    src_t, dst_t = pair
    x = C.source(src_t, 65).reshape(1, 5, 13)
    m = _model(C.raw_cast((1, 5, 13), src_t, dst_t))
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, 0)
    assert ex.LaunchKernels(key) == (["copy"] if src_t == dst_t else ["cast_host"])
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = x
    assert ex.ExecuteSubgraph(key).ok()
    got = ex.GetTensorView(key, ex.GetOutputs(key)[0]).GetData()
    assert got.dtype == np.dtype(dst_t) and got.tobytes() == C.cast_ref(x, dst_t).tobytes()


@pytest.mark.parametrize("name", sorted(C.REFUSALS))
def test_refusals_say_why(name):
    build, reason = C.REFUSALS[name]
    m = _model(build())
    for flag in (DeviceFlag.kCPU, DeviceFlag.kGPU):
        ex = HipModelExecutor(0, 0 if flag == DeviceFlag.kCPU else 1, flag)
        assert ex.InvestigateModelSpec(m).unsupported_ops[flag] != set(), name
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    st = ex.PrepareSubgraph(m)
    assert not st.ok() and reason in st.message(), st.message()


def test_launcher_check_says_why():
    lib = _abi.load()
    x = np.zeros(8, np.float32)
    y = np.zeros(8, np.int32)
    for change, reason in ((dict(input=None), "null pointer"), (dict(count=-1), "negative count"),
                           (dict(out_type=0), "types must be"), (dict(input=x.ctypes.data + 1), "not aligned")):
        p = _abi.CastParams(4, 2, 8, x.ctypes.data, y.ctypes.data)
        for k, v in change.items():
            setattr(p, k, v)
        assert lib.bh_cast(ctypes.byref(p), None) != 0
        msg = lib.bh_last_error().decode()
        assert msg.startswith("bh_cast: ") and reason in msg, msg


# ---- the padded text models ---------------------------------------------------------------------------
def _compare(name, t, got, ref):
    assert got.dtype == ref.dtype, (name, t)
    if ref.dtype == np.float32:
        assert_float_close(got, ref, "%s tensor %d" % (name, t))
    else:
        np.testing.assert_array_equal(got.reshape(ref.shape), ref, err_msg="%s tensor %d" % (name, t))


def test_the_mask_chain_is_what_the_builder_says():
    om = OModel(C.PADDED["padded_text_i8"]())
    names = [o.builtin for o in om.operators][:5]
    assert names == [53, 41, 18, 114, 22]  # CAST, SUB, MUL, QUANTIZE, RESHAPE
    assert [tuple(om.tensors[t].shape) for t in om.inputs] == [(2, 17), (2, 17)]
    q = om.tensors[om.operators[3].outputs[0]]
    assert (float(q.scale[0]), int(q.zero_point[0])) == (float(np.float32(10000.0 / 255)), 127)
    mask4 = om.operators[4].outputs[0]
    assert tuple(om.tensors[mask4].shape) == (2, 1, 1, 17)
    assert sum(mask4 in o.inputs for o in om.operators) == 2  # one mask feeds both blocks
    assert [o.builtin for o in OModel(C.PADDED["padded_text_f32"]()).operators if o.builtin in (53, 114)] == [53]


@pytest.mark.parametrize("name", sorted(C.PADDED))
def test_padded_text_models_on_cpu_executor_every_tensor(name):
    buf = C.PADDED[name]()
    om = OModel(buf)
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    spec = ex.InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kCPU] == set() and spec.unsupported_ops[DeviceFlag.kGPU] == set()
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, 0)
    views = {t.index: ex.GetTensorView(key, t.index) for t in om.tensors if not t.is_const}
    x = C.inputs(buf, 0)
    assert [int((v == 0).sum()) for v in x[om.inputs[1]]] == [5, 0]
    ref = run_reference(buf, x, table=C.REF_TABLE)
    for t, v in x.items():
        views[t].GetData()[...] = v
    assert ex.ExecuteSubgraph(key).ok()
    for t, v in views.items():
        _compare(name, t, v.GetData(), ref[t])
    if name.endswith("i8"):  # a masked key's score saturates at the bottom of the range
        from tests import mask_models as M
        for sc, ms, pr, ctx, bias in M.masked_attention_tensors(buf):
            b = np.broadcast_to(ref[bias], ref[ms].shape)
            assert (b == -128).any() and (ref[ms][b == -128] == -128).all()


@pytest.mark.parametrize("name", ["padded_text_i8", "padded_text_hybrid"])
def test_padded_text_models_job_batches_on_cpu(name):
    """the mask's axis 0 is the job axis"""
    buf = C.PADDED[name](batch=1)
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(0, 0)
    st = ex.PrepareJobBatches(m, key, 3)
    assert st.ok(), st.message()
    xs = [C.inputs(buf, s) for s in range(3)]
    refs = [run_reference(buf, x, table=C.REF_TABLE) for x in xs]
    for n in (2, 3):
        for s in range(n):
            for t, v in xs[s].items():
                ex.GetJobSlotView(key, t, n, s).GetData()[...] = v
        assert ex.ExecuteJobBatch(key, n).ok()
        for s in range(n):
            for t in ex.GetOutputs(key):
                _compare(name, t, ex.GetJobSlotView(key, t, n, s).GetData().reshape(refs[s][t].shape), refs[s][t])


def masked_ids_leave_the_logits_alone(flag, worker):
    """The float32 padded model, exactly: other ids at the masked positions leave the class logits bit-identical.
    The shapes are equal, so every reduction runs in the same order; expf of a score 10,000 below the row maximum is
    exactly 0, so the masked terms are exact zeros both times.  First, on the reference: the two runs' embedding
    rows differ at the masked positions."""
    buf = C.PADDED["padded_text_f32"]()
    om = OModel(buf)
    t_ids, t_mask = om.inputs
    x0 = C.inputs(buf, 0)
    x1 = {t_ids: x0[t_ids].copy(), t_mask: x0[t_mask]}
    masked = x0[t_mask] == 0
    assert masked[0].sum() == 5 and masked[1].sum() == 0
    x1[t_ids][masked] = (x0[t_ids][masked] + 1 + np.arange(masked.sum())) % 128
    assert (x1[t_ids][masked] != x0[t_ids][masked]).all()
    look = next(o for o in om.operators if o.builtin == 7)
    r0, r1 = (run_reference(buf, x, table=C.REF_TABLE)[look.outputs[0]] for x in (x0, x1))
    assert (r0[masked] != r1[masked]).any(-1).all() and (r0[~masked] == r1[~masked]).all()
    m = HipModel(0)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(0, worker, flag)
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, worker)
    outs = []
    for x in (x0, x1):
        for t, v in x.items():
            ex.GetTensorView(key, t).GetData()[...] = v
        assert ex.ExecuteSubgraph(key).ok()
        outs.append(ex.GetTensorView(key, ex.GetOutputs(key)[0]).GetData().copy())
    assert np.isfinite(outs[0]).all() and outs[0].shape[0] == 2
    # item 1 has no masked token and unchanged ids; item 0's logits come from token 0, which sees the five
    # changed tokens only through keys that are masked
    assert outs[0].view(np.uint32).tobytes() == outs[1].view(np.uint32).tobytes()


def test_masked_ids_leave_the_logits_alone():
    from band_amd import backend  # noqa: F401
    masked_ids_leave_the_logits_alone(DeviceFlag.kCPU, 0)


def test_host_code_under_sanitizers(tmp_path):
    """tests/native/cast_test.cc: CpuCast over the 16 pairs on exactly sized, misaligned heap buffers with the
    extreme values, and CastArgs on the refused and one good model, under AddressSanitizer and UBSan"""
    csrc = os.path.join(ROOT, "band_amd", "csrc")
    models = {name: build() for name, (build, _) in C.REFUSALS.items()}
    models["good_cast"] = C.raw_cast((1, 8), np.int32, np.float32)
    paths = []
    for name, buf in models.items():
        paths.append(str(tmp_path / (name + ".tflite")))
        with open(paths[-1], "wb") as f:
            f.write(buf)
    exe = str(tmp_path / "cast_test")
    src = [os.path.join(ROOT, "tests", "native", "cast_test.cc")] + [
        os.path.join(csrc, "backend", "hip", f) for f in ("tflite_reader.cc", "lower_args.cc", "quant.cc", "cpu_kernels.cc")]
    src.append(os.path.join(csrc, "compat", "band", "common.cc"))
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unused-function", "-ffp-contract=off",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I" + os.path.join(ROOT, "include"),
                    "-I" + os.path.join(csrc, "compat"), "-I" + csrc] + src + ["-o", exe, "-lpthread"], check=True,
                   timeout=600)
    r = subprocess.run([exe] + paths, capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "cast ok" in r.stdout, r.stdout
    lines = r.stdout.splitlines()
    for name, (_, reason) in C.REFUSALS.items():
        hit = [ln for ln in lines if "/%s.tflite op 0 " % name in ln]
        assert len(hit) == 1 and reason in hit[0], (name, hit)
    assert [ln for ln in lines if "/good_cast.tflite op 0 " in ln and ln.endswith(": ok")], lines
