"""The masked form of the fused attention launch without a GPU: the composed
reference of tests.mask_models judged alone (the saturation case's shares, four
wrong variants that must each show, the padding rows, the identity bias on the
sum-order rows), the case set's coverage, every refusal bh_attention_i8_check
adds for a bias with its reason, and the name and LDS of a launch with and
without one.

Expected values come from the oracle (FULLY_CONNECTED per slice, add, softmax);
nothing here runs the kernel."""
import ctypes

import numpy as np
import pytest

from band_amd import _abi
from tests import attention_models as A
from tests import mask_models as M

CASES = M.launcher_cases()


# ---- the reference judged alone -----------------------------------------------------------------
def test_saturation_case_shares():
    """A float simulation (scores 1.2 wide, bias uniform over +-10.2, window +-6.4) puts about a fifth of the masked
    scores at each bound.  The issue's case has the bias at scale 0.1; it is at 0.08 here because at equal input
    scales the ADD's two input multipliers are equal and exchanging them (a variant below) is no mistake."""
    c = M.saturation_case()
    m = c.masked()
    lo, hi = (m == -128).mean(), (m == 127).mean()
    print("saturates: %.1f %% at -128, %.1f %% at 127, %.1f %% inside" % (100 * lo, 100 * hi, 100 * (1 - lo - hi)))
    assert lo >= 0.10 and hi >= 0.10 and 1 - lo - hi >= 0.25
    s = c.scores().astype(np.int32)
    width = (s.max(-1) - s.min(-1)).mean()
    print("saturates: a row of scores is %.1f LSBs wide on average" % width)
    assert (c.keys, c.rows, c.head_dim) == (70, 33, 65) and c.bias.min() == -128 and c.bias.max() == 127


def _variants(c):
    s = c.scores()
    ma, sa, mb, sb, mo, so, left = [int(v) for v in c.add_consts()]
    out = {"bias_dropped": c.masked(s, bias=np.full_like(c.bias, c.z_b)),
           "multipliers_exchanged": c.masked(s, consts=np.array([mb, sb, ma, sa, mo, so, left], np.int32)),
           "batch_0_bias_everywhere": c.masked(s, bias=np.broadcast_to(c.bias[:1], c.bias.shape).copy())}
    return s, out


def test_wrong_variants_show_in_the_reference():
    """the bias dropped, the two input multipliers exchanged, batch 0's bias for every batch: each changes at least a
    quarter of the masked scores and at least one byte of the context"""
    c = M.saturation_case()
    s, variants = _variants(c)
    right = c.masked(s)
    ctx = c.ctx(right)
    for name, wrong in variants.items():
        share = (wrong != right).mean()
        changed = (c.ctx(wrong) != ctx).sum()
        print("%s: %.1f %% of the masked scores, %d context bytes" % (name, 100 * share, changed))
        assert share >= 0.25 and changed >= 1, name


def test_a_bias_along_rows_instead_of_keys_shows():
    """a [b0, 1, 1, keys] bias read as [b0, 1, rows, 1]"""
    c = M.saturation_case()
    vec = c.bias[:, :1, :1, :].copy()
    s = c.scores()
    right = c.masked(s, bias=vec)
    wrong = c.masked(s, bias=np.ascontiguousarray(vec.reshape(c.batch[0], 1, c.keys, 1)[:, :, :c.rows]))
    share = (wrong != right).mean()
    changed = (c.ctx(wrong) != c.ctx(right)).sum()
    print("rows_for_keys: %.1f %% of the masked scores, %d context bytes" % (100 * share, changed))
    assert share >= 0.25 and changed >= 1


def test_padding_rows():
    """every key masked: every masked score is -128 and the probabilities are equal; keys masked from PAD_FROM on:
    their probabilities are at most those of every unmasked key"""
    c = M.padding_case()
    m = c.masked()
    p = c.probs(m)
    assert (m[0] == -128).all()
    assert (p[0] == p[0][..., :1]).all() and (p[0] > -128).all()
    assert (m[1][..., M.PAD_FROM:] == -128).all() and (m[1][..., :M.PAD_FROM] == c.scores()[1][..., :M.PAD_FROM]).all()
    assert (p[1][..., M.PAD_FROM:].max(-1) <= p[1][..., :M.PAD_FROM].min(-1)).all()


def test_identity_bias_keeps_the_sum_order_rows():
    c, rev_rows, pair_rows = M.identity_case()
    s = c.scores()
    np.testing.assert_array_equal(c.masked(s), s)
    base = A.sum_order()[0]
    np.testing.assert_array_equal(c.ref(), base.ref())
    assert len(rev_rows) >= A.SUM_ORDER_FLOOR and len(pair_rows) >= A.SUM_ORDER_FLOOR
    ref = c.probs(s)[0, 0]
    assert (A.np_softmax(s[0, 0], c.in_scale, "reversed") != ref).any(-1)[rev_rows].all()
    assert (A.np_softmax(s[0, 0], c.in_scale, "pairwise") != ref).any(-1)[pair_rows].all()


def test_case_set_covers_the_issues_values():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    by = {c.name: c for c in CASES}
    for layout in M.LAYOUTS:
        c = by["layout_" + layout]
        assert (c.batch, c.rows, c.keys, c.head_dim, c.out_dim) == ((2, 3), 17, 33, 36, 36)
        assert c.bias.shape == M.bias_shape(layout, (2, 3), 17, 33)
    assert {by["keys_%d" % k].keys for k in M.KEYS} == set(M.KEYS)
    assert all(by["keys_%d" % k].rows == 17 and by["keys_%d" % k].bias.shape[2:] == (17, k) for k in M.KEYS)
    assert (by["keys_1024_rows_65"].keys, by["keys_1024_rows_65"].rows) == (1024, 65)
    assert {by["bias_off_1"].bias_off, by["bias_off_4"].bias_off} == {1, 4}
    assert by["heads_layout"].layout == "heads" and by["scores_second"].operand == 1
    assert by["narrow_window"].act == (-20, 41)
    # both load forms: dwords need keys % 4 == 0, an aligned base and strides that are multiples of 4
    assert {c.keys % 4 == 0 and c.bias_off % 4 == 0 and c.bias.shape[3] > 1 for c in CASES} == {False, True}
    # the ADD blocks hold what the launcher takes
    for c in CASES:
        ma, sa, mb, sb, mo, so, left = [int(v) for v in c.add_consts()]
        assert sa <= 0 and sb <= 0 and -31 <= so <= 0 and 0 <= left <= 31, c.name


# ---- the launcher's checks -------------------------------------------------------------------------
@pytest.mark.parametrize("name,change,reason", M.refused_params(), ids=[r[0] for r in M.refused_params()])
def test_bias_parameter_checks_say_why(name, change, reason):
    from band_amd import backend  # noqa: F401
    lib = _abi.load()
    p, bufs, _ = M.prepare(M.valid_case(), device=False)
    assert lib.bh_attention_i8_check(ctypes.byref(p)) == 0, lib.bh_last_error()
    assert lib.bh_attention_i8_kernel(ctypes.byref(p)) == M.KERNEL.encode()
    change(p)
    assert lib.bh_attention_i8_check(ctypes.byref(p)) != 0
    msg = lib.bh_last_error().decode()
    assert msg.startswith("bh_attention_i8: ") and reason in msg, msg
    assert lib.bh_attention_i8_kernel(ctypes.byref(p)) == b""
    assert lib.bh_attention_i8_lds_bytes(ctypes.byref(p)) == 0


def test_the_unmasked_forms_refusals_hold_with_a_bias():
    from band_amd import backend  # noqa: F401
    lib = _abi.load()
    for name, change, reason in A.refused_params():
        p, bufs, _ = M.prepare(M.valid_case(), device=False)
        change(p)
        assert lib.bh_attention_i8_check(ctypes.byref(p)) != 0, name
        assert reason in lib.bh_last_error().decode(), name


def test_name_and_lds_with_and_without_a_bias():
    """zeroed new fields: the unmasked kernel, whatever the ADD block would refuse; a bias: the masked kernel's
    name; the direct form of the ADD takes no LDS of its own"""
    from band_amd import backend  # noqa: F401
    lib = _abi.load()
    p, bufs, _ = A.prepare(A.valid_case(), device=False)
    assert not p.bias and p.bias_key_stride == 0 and p.add.left_shift == 0 and p.add_scores_operand == 0
    assert lib.bh_attention_i8_kernel(ctypes.byref(p)) == A.KERNEL.encode()
    plain = lib.bh_attention_i8_lds_bytes(ctypes.byref(p))
    assert plain == 64 * 80 + 128 * 80 + 1024
    p.add.a_shift, p.bias_key_stride = 3, 2  # ignored without a bias
    assert lib.bh_attention_i8_kernel(ctypes.byref(p)) == A.KERNEL.encode()
    pm, bufs_m, _ = M.prepare(M.valid_case(), device=False)
    assert lib.bh_attention_i8_kernel(ctypes.byref(pm)) == M.KERNEL.encode()
    for keys, strip in ((1, 64 * 80), (65, 64 * 144), (1024, 64 * 1040)):
        pm.keys = keys
        pm.bias_key_stride, pm.bias_row_stride, pm.bias_bstride[1] = 0, 0, 0
        assert lib.bh_attention_i8_lds_bytes(ctypes.byref(pm)) == strip + 128 * 80 + 1024


# ---- the synthesiser and the models --------------------------------------------------------------
# sha256 of the bytes the builders emitted before _attention took a bias
DIGESTS = {
    "attention_block_i8": "b345bb954efabd54c03fffd781f20b56abb5ee468c879c9b656e545db7705256",
    "attention_block_f32": "6fe6a344961cbfc01da08e5a12e2615b022bfbb03bc4dd4280f3279448280082",
    "attention_block_hybrid": "36791600cc705b22755e95993d7f652fabbb8b9f1467b745e803b336d4622dcd",
    "encoder_block_i8": "e9e552e8995cf3c977e454f64ade9b6c2284e004e51a0bec5478a520e82840b4",
    "vit_tiny_i8": "ac28ab83d6eec0efd55ee60610a164da5a77ef781ad3d205bb2fff640f294d08",
    "vit_tiny_ln_mlp_i8": "5a204569f9b2aae7141aa33809422d6a7a08e85b303af5d828bb9c226d5d45eb",
    "text_encoder_i8": "e5e67299bb7aca19981ee7d3db1e320a13b0caa9be9044b4d6ef81df37343e0e",
    "text_encoder_f32": "add02f55a3fb10d6085d5762ed22f15efcd85dabc7dc4d67255cda3730bc58f4",
    "attention_block_u8": "1c9b05309eb856acd3b12cbad06c768adbc6184dfde033ce5ce2d84ffb092ed7",
}


def test_existing_builders_emit_the_bytes_they_did():
    import hashlib
    from band_amd.tflite_synth import attention_block, encoder_block, text_encoder, vit_tiny
    built = {
        "attention_block_i8": attention_block(np.int8, tokens=17, dim=48, heads=3),
        "attention_block_f32": attention_block(np.float32, tokens=17, dim=48, heads=3),
        "attention_block_hybrid": attention_block(np.float32, tokens=17, dim=48, heads=3, hybrid="symmetric"),
        "encoder_block_i8": encoder_block(np.int8, tokens=17, dim=48, heads=3, hidden=96),
        "vit_tiny_i8": vit_tiny(np.int8, size=32, dim=48, heads=3),
        "vit_tiny_ln_mlp_i8": vit_tiny(np.int8, size=32, dim=48, heads=3, layer_norm=True, mlp=True),
        "text_encoder_i8": text_encoder(np.int8, tokens=17, dim=48, heads=3, hidden=96, vocab=128, batch=2),
        "text_encoder_f32": text_encoder(np.float32, tokens=17, dim=48, heads=3, hidden=96, vocab=128),
        "attention_block_u8": attention_block(np.uint8, tokens=17, dim=48, heads=3),
    }
    assert {k: hashlib.sha256(bytes(v)).hexdigest() for k, v in built.items()} == DIGESTS


def _cpu_exec(buf, mid=0):
    from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
    from band_amd import backend  # noqa: F401
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(mid, 0, DeviceFlag.kCPU)
    assert ex.InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kCPU] == set()
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    ex._model_ref = m
    return m, ex, SubgraphKey(mid, 0)


def test_masks_are_what_the_builders_say():
    from oracle.tflite_fb import Model as OModel
    for name, shape in (("causal_17_48_3", (1, 1, 17, 17)), ("relative_17_48_3", (1, 3, 17, 17))):
        buf = M.MODELS[name]()
        om = OModel(buf)
        (sc, ms, pr, ctx, bias), = M.masked_attention_tensors(buf)
        t = om.tensors[bias]
        assert t.is_const and tuple(t.shape) == shape and t.np_dtype == np.int8, name
        q = lambda i: (float(om.tensors[i].scale[0]), int(om.tensors[i].zero_point[0]))
        assert q(ms) == q(sc)
        if name.startswith("causal"):
            b = np.asarray(t.data).reshape(17, 17)
            assert (b[np.tril_indices(17)] == 127).all() and (b[np.triu_indices(17, 1)] == -128).all()
            assert q(bias) == (float(np.float32(10000.0 / 255)), 127)
        else:
            assert q(bias) == q(sc) and t.data.min() == -128 and t.data.max() == 127


@pytest.mark.parametrize("name", sorted(M.MODELS))
def test_models_on_the_cpu_executor(monkeypatch, name):
    """every tensor viewed, against run_reference; the flag is set and ignored; a masked key's score is -128 and its
    probability the row's smallest"""
    from oracle.tflite_fb import Model as OModel
    from tests.graph_reference import run_reference
    monkeypatch.setenv("BAND_HIP_FUSED_ATTENTION", "1")
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf = M.MODELS[name]()
    om = OModel(buf)
    m, ex, key = _cpu_exec(buf)
    assert M.KERNEL not in ex.LaunchKernels(key) and A.KERNEL not in ex.LaunchKernels(key)
    views = {t.index: ex.GetTensorView(key, t.index) for t in om.tensors if not t.is_const}
    for seed in (1, 0):  # (seed 0 last: its first batch item has masked tokens)
        x = M.model_inputs(buf, seed)
        ref = run_reference(buf, x)
        for t, v in x.items():
            views[t].GetData()[...] = v
        assert ex.ExecuteSubgraph(key).ok()
        for t, v in views.items():
            np.testing.assert_array_equal(v.GetData().reshape(ref[t].shape), ref[t], err_msg="%s tensor %d" % (name, t))
    (sc, ms, pr, ctx, bias), = M.masked_attention_tensors(buf)
    if name.startswith(("causal", "padded")):
        b = np.broadcast_to(ref[bias] if bias in ref else om.tensors[bias].data, ref[ms].shape)
        assert (b == -128).any() and (ref[ms][b == -128] == -128).all()
        assert (np.where(b == -128, ref[pr], -128).max(-1) <= np.where(b == -128, 127, ref[pr]).min(-1)).all()


@pytest.mark.parametrize("name", ["causal_17_48_3", "padded_one_17_48_3"])
def test_models_job_batches_on_the_cpu_executor(name):
    """job batches 2 and 3 against single runs; the padding mask's axis 0 is the job axis"""
    from tests.graph_reference import run_reference
    buf = M.MODELS[name]()
    m, ex, key = _cpu_exec(buf)
    st = ex.PrepareJobBatches(m, key, 3)
    assert st.ok(), st.message()
    xs = [M.model_inputs(buf, s) for s in range(3)]
    refs = [run_reference(buf, x) for x in xs]
    for n in (2, 3):
        for s in range(n):
            for t, v in xs[s].items():
                ex.GetJobSlotView(key, t, n, s).GetData()[...] = v
        assert ex.ExecuteJobBatch(key, n).ok()
        for s in range(n):
            for t in ex.GetOutputs(key):
                got = ex.GetJobSlotView(key, t, n, s).GetData()
                np.testing.assert_array_equal(got.reshape(refs[s][t].shape), refs[s][t], err_msg="%s n=%d slot %d" % (name, n, s))


def float_causal_rows_ignore_later_tokens(flag, worker):
    """The float32 causal block, exactly: changing the input at tokens from `cut` on leaves the output rows before
    `cut` bit-identical.  The shapes are equal, so every reduction runs in the same order; expf of a score 10,000
    below the row maximum is exactly 0, so the masked terms of P V are exact zeros both times."""
    from band_amd import HipModel, HipModelExecutor, SubgraphKey
    from band_amd.tflite_synth import attention_block
    buf = attention_block(np.float32, tokens=17, dim=48, heads=3, attention_bias="causal")
    m = HipModel(0)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(0, worker, flag)
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, worker)
    rng = np.random.default_rng(3)
    x0 = rng.normal(0, 1, (1, 17, 48)).astype(np.float32)
    x1 = x0.copy()
    cut = 9
    x1[:, cut:] = rng.normal(0, 1, (1, 17 - cut, 48)).astype(np.float32)
    outs = []
    for x in (x0, x1):
        ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = x
        assert ex.ExecuteSubgraph(key).ok()
        outs.append(ex.GetTensorView(key, ex.GetOutputs(key)[0]).GetData().reshape(1, 17, 48).copy())
    assert (x0[:, cut:] != x1[:, cut:]).all() and (outs[0][:, cut:] != outs[1][:, cut:]).any()
    assert np.isfinite(outs[0]).all()
    np.testing.assert_array_equal(outs[0][:, :cut].view(np.uint32), outs[1][:, :cut].view(np.uint32))


def test_float_causal_rows_ignore_later_tokens():
    from band_amd import DeviceFlag
    from band_amd import backend  # noqa: F401
    float_causal_rows_ignore_later_tokens(DeviceFlag.kCPU, 0)


def test_attention_check_under_sanitizers(tmp_path):
    """tests/native/attn_check_test.cc: bh_attention_i8's check (band_hip_attention_shared.h, pure host code) on a
    valid block, every refusal the bias adds, and INT64_MAX / INT64_MIN / 2^31 in every stride field, under
    AddressSanitizer and UBSan as a stand-alone program"""
    import os
    import subprocess
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    exe = str(tmp_path / "attn_check_test")
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I" + os.path.join(root, "include"), os.path.join(root, "tests", "native", "attn_check_test.cc"), "-o", exe],
                   check=True, timeout=600)
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "Sanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]
    assert "attn check ok" in r.stdout, r.stdout
