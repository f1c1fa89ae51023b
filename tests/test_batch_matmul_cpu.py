"""BATCH_MATMUL without a GPU: the references themselves, the conditions on
the case set, CpuBatchMatMul through the C ABI on every launcher case, the
refusals, attention_block / vit_tiny on the kCPU executor and the job-batch
rule.  The reference is the oracle's FULLY_CONNECTED per batch slice
(tests/bmm_models.py); int8 tensors are compared with assert_array_equal, float
launcher cases at gamma(K + 2) sum|a||b| + 2^-126, float models at the tolerance
of tests/test_float_cpu.py."""
import ctypes

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi
from band_amd.tflite_reader_py import OPTION_FIELDS, read
from band_amd.tflite_synth import OPT
from tests import bmm_models as B
from tests import float_harness as H
from tests import reindex_models as R
from tests.graph_reference import run_reference
from tests.grouped_models import HostBuffer
from tests.test_float_cpu import assert_float_close

CASES = B.launcher_cases()
FLOAT_CASES = B.float_cases()


@pytest.fixture(scope="module")
def refs():
    """bmm_ref of every launcher case, computed once"""
    return {c.name: B.bmm_ref(c) for c in CASES + FLOAT_CASES}


def _model(buf, mid=0):
    m = HipModel(mid)
    assert m.FromBuffer(buf).ok()
    return m


def _share(a, b):
    assert a.shape == b.shape
    return float((a != b).mean())


# ---- the references can tell mistakes apart ------------------------------------
def test_numpy_restatement_equals_the_oracle(refs):
    """np_bmm (the folded form in numpy) is the oracle's FULLY_CONNECTED per slice, on every int8 case"""
    for c in CASES:
        np.testing.assert_array_equal(B.np_bmm(c), refs[c.name], err_msg=c.name)


def test_references_tell_wrong_variants_apart(refs):
    """Each wrong variant differs from bmm_ref on >= 25 % of the elements of the
    cases where it applies; the smallest share is printed (measured: 0.66 over
    the five arithmetic / layout variants).

    The half-up step-2 rounding differs from TFLite's rounding exactly on the
    negative step-2 ties and nowhere else; on the issue's two tie cases those
    are 40 of 561 outputs each, so its >= 25 % is held on negative_tie_case,
    which is built of them (measured: 0.50).  On all three the difference is
    also asserted as the exact set: every unclamped negative tie differs by
    one, nothing else differs, at least 20 do."""
    shares = {}

    def note(kind, c, wrong):
        s = _share(wrong, refs[c.name])
        shares.setdefault(kind, []).append((s, c.name))

    def spread_out(c):  # a saturated reference hides arithmetic mistakes
        r = refs[c.name].astype(np.int32)
        return ((r > -128) & (r < 127)).mean() >= 0.5

    for c in CASES:
        m, n, k = c.mnk
        if "extreme" in c.name or c.name == "negative_ties":
            continue
        square = c.rhs.shape[-1] == c.rhs.shape[-2]
        if square and n >= 15:
            note("adj_y", c, B.np_bmm(c, "adj_y"))
        if c.z_l != 0 and k >= 15 and n >= 15 and spread_out(c):
            note("no_colsum", c, B.np_bmm(c, "no_colsum"))
        if c.z_l != 0 and c.z_r != 0 and k >= 15 and spread_out(c) and m * n >= 15:
            note("no_kzz", c, B.np_bmm(c, "no_kzz"))
            if k % 64 and abs((-(-k // 64) * 64 - k) * c.z_l * c.z_r * c.mult / 2.0 ** (31 - c.shift)) >= 4:
                note("padded_k", c, B.np_bmm(c, "padded_k"))  # a K pad worth >= 4 output LSBs
        rl = tuple(c.rhs.shape[:-2])
        if int(np.prod(rl)) > 1 and spread_out(c):
            note("slice0", c, B.np_bmm(c, "slice0"))
    for kind in ("adj_y", "no_colsum", "no_kzz", "padded_k", "slice0"):
        assert kind in shares and len(shares[kind]) >= 2, (kind, shares.get(kind))
        low = min(shares[kind])
        print("wrong variant %-10s applies to %2d cases, smallest share %.3f (%s)" % (kind, len(shares[kind]), *low))
        assert low[0] >= 0.25, (kind, low)
    # half-up step 2: >= 25 % on the case built of negative ties, and on every tie case the exact set
    c = B.negative_tie_case()
    share = _share(B.np_bmm(c, "half_up"), refs[c.name])
    print("wrong variant half_up    on %s: share %.3f" % (c.name, share))
    assert share >= 0.25, share
    for c in B.tie_cases() + [B.negative_tie_case()]:
        acc, x = B.step1(c)
        ref = refs[c.name].astype(np.int32)
        wrong = B.np_bmm(c, "half_up").astype(np.int32)
        neg_tie = ((x & 7) == 4) & (x < 0)
        neg_tie = neg_tie.reshape(ref.shape) & (ref > -128) & (ref < 127)
        np.testing.assert_array_equal(wrong != ref, neg_tie, err_msg=c.name)
        assert (wrong - ref)[neg_tie].tolist() == [1] * int(neg_tie.sum()) and neg_tie.sum() >= 20
        print("wrong variant half_up    on %s: %d of %d differ (share %.3f)" % (c.name, neg_tie.sum(), ref.size,
                                                                                   neg_tie.mean()))


# ---- conditions on the case set, asserted on the reference alone ---------------
def test_tie_cases_hold_ties_of_both_signs(refs):
    for c in B.tie_cases():
        assert (c.mult, c.shift) == (1 << 30, -3)
        assert np.abs(c.lhs.astype(int) - c.z_l).max() <= 3 and np.abs(c.rhs.astype(int) - c.z_r).max() <= 3
        acc, x = B.step1(c)
        tie = (x & 7) == 4
        neg, pos = int((tie & (x < 0)).sum()), int((tie & (x >= 0)).sum())
        print("%s: %d negative and %d positive step-2 ties of %d outputs" % (c.name, neg, pos, x.size))
        assert x.size == 561 and neg >= 20 and pos >= 20


def test_left_shift_case_stays_inside(refs):
    c = B.left_shift_case()
    r = refs[c.name].astype(np.int32)
    inside = float(((r > -128) & (r < 127)).mean())
    print("left shift: shift %+d, %.0f %% of the outputs unclamped" % (c.shift, 100 * inside))
    assert c.shift == 2 and inside >= 0.25


def test_clamp_case_reaches_both_ends(refs):
    c = B.clamp_case()
    r = refs[c.name].astype(np.int32)
    lo, hi = float((r == -128).mean()), float((r == 127).mean())
    inside = float(((r > -128) & (r < 127)).mean())
    print("clamps: shift %+d, %.1f %% at -128, %.1f %% at 127, %.1f %% inside" % (c.shift, 100 * lo, 100 * hi, 100 * inside))
    assert c.shift < 0 and lo >= 0.05 and hi >= 0.05 and inside >= 0.25


def test_both_requantisation_forms_occur():
    lib = _abi.load()
    ok = {c.name: B.fast_ok(c, lib) for c in CASES}
    assert set(ok.values()) == {0, 1}, ok
    assert ok["left_shift"] == 0 and ok["clamps"] == 1


def test_case_set_covers_the_issues_values():
    trip = B.covering_triples()
    assert {(m, n) for m, n, k in trip} == {(m, n) for m in B.MS for n in B.NS}
    assert {(m, k) for m, n, k in trip} == {(m, k) for m in B.MS for k in B.KS}
    assert {n for m, n, k in trip} == set(B.NS) and {k for m, n, k in trip} == set(B.KS)


# ---- the host twins ----------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_cpu_batch_matmul_launcher_cases(refs, case):
    from band_amd import backend  # noqa: F401  (registers the bhx_* symbols)
    got = B.launch(case, _abi.load(), device=False)
    np.testing.assert_array_equal(got, refs[case.name])


@pytest.mark.parametrize("case", FLOAT_CASES, ids=[c.name for c in FLOAT_CASES])
def test_cpu_batch_matmul_f32_launcher_cases(refs, case):
    from band_amd import backend  # noqa: F401
    ref, tol = refs[case.name]
    H.check(B.launch(case, _abi.load(), device=False), ref, tol, case.name)


@pytest.mark.parametrize("name,change,reason", B.refused_params(), ids=[r[0] for r in B.refused_params()])
def test_parameter_checks_say_why(name, change, reason):
    from band_amd import backend  # noqa: F401
    lib = _abi.load()
    bufs = [HostBuffer(np.zeros(64, np.uint8)) for _ in range(3)]
    p = B.valid_params(*(b.value for b in bufs))
    assert lib.bh_batch_matmul_check(ctypes.byref(p), 1) == 0
    assert lib.bh_batch_matmul_i8_kernel(ctypes.byref(p)) == B.KERNEL.encode()
    change(p)
    assert lib.bh_batch_matmul_check(ctypes.byref(p), 1) != 0
    msg = lib.bh_last_error().decode()
    assert msg.startswith("bh_batch_matmul_i8: ") and reason in msg, msg
    assert lib.bh_batch_matmul_i8_kernel(ctypes.byref(p)) == b""
    assert lib.bhx_cpu_batch_matmul(ctypes.byref(p), 0) != 0
    if name != "k_limit":  # float32 has no K limit
        assert lib.bh_batch_matmul_check(ctypes.byref(p), 4) != 0
        assert lib.bh_last_error().decode().startswith("bh_batch_matmul_f32: ")


# ---- the op's refusals ---------------------------------------------------------------
REFUSALS = {
    "uint8": (lambda: B.one_op_model((1, 4, 8), (1, 8, 5), np.uint8), "int8 and float32 only"),
    "int16": (lambda: B.one_op_model((1, 4, 8), (1, 8, 5), np.int16), "int8 and float32 only"),
    "hybrid": (lambda: B.one_op_model((1, 4, 8), (1, 8, 5), np.float32, rhs_dtype=np.int8), "hybrid BATCH_MATMUL"),
    "rank5": (lambda: B.one_op_model((1, 1, 2, 4, 8), (1, 1, 2, 8, 5)), "rank 2 to 4"),
    "mismatched_k": (lambda: B.one_op_model((1, 4, 8), (1, 7, 5)), "mismatched K"),
    "k_limit": (lambda: B.one_op_model((1, 2, 32768), (1, 32768, 2)), "K > 32767"),
    "mixed_types": (lambda: B.one_op_model((1, 4, 8), (1, 8, 5), np.int8, out_dtype=np.float32), "differ in type"),
    "batch_dims": (lambda: B.one_op_model((2, 4, 8), (3, 8, 5), out_shape=[2, 4, 5]), "neither equal nor 1"),
    # the launchers' limits, refused by the support check already
    "batch_dim_limit": (lambda: B.one_op_model((65536, 1, 2), (1, 2, 1)), "a batch dim above 65535"),
    "index_range": (lambda: B.one_op_model((2, 40000, 30000), (30000, 2), np.float32), "2^31 or more elements"),
}


@pytest.mark.parametrize("name", sorted(REFUSALS))
def test_refusals_say_why(name):
    """the op is in unsupported_ops of the worker, and the lowering error names the reason"""
    build, reason = REFUSALS[name]
    m = _model(build())
    spec = HipModelExecutor(0, 0, DeviceFlag.kCPU).InvestigateModelSpec(m)
    assert spec.unsupported_ops[DeviceFlag.kCPU] == {0}
    st = HipModelExecutor(0, 0, DeviceFlag.kCPU).PrepareSubgraph(m)
    assert not st.ok() and reason in st.message(), st.message()


# ---- models on the kCPU executor ---------------------------------------------------------
def _compare(name, t, got, ref):
    assert got.dtype == ref.dtype, (name, t)
    if ref.dtype == np.float32:
        assert_float_close(got, ref, "%s tensor %d" % (name, t))
    else:
        np.testing.assert_array_equal(got.reshape(ref.shape), ref, err_msg="%s tensor %d" % (name, t))


def non_constant_tensors(buf):
    return [i for i, t in enumerate(read(buf)["tensors"]) if t["data"] is None]


@pytest.fixture(scope="module")
def model_refs():
    out = {}
    for name, build in B.MODELS.items():
        buf = build()
        xs = [R.zoo_input(buf, seed=30 + s) for s in range(3)]
        out[name] = (buf, xs, [run_reference(buf, x) for x in xs])
    return out


@pytest.mark.parametrize("name", sorted(B.MODELS))
def test_models_on_cpu_executor_every_tensor(model_refs, name):
    buf, xs, refs_ = model_refs[name]
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kCPU] == set()
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, 0)
    assert any(o["builtin"] == B.BATCH_MATMUL for o in read(buf)["ops"])
    views = {t: ex.GetTensorView(key, t) for t in non_constant_tensors(buf)}
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = xs[0]
    assert ex.ExecuteSubgraph(key).ok()
    for t, v in views.items():
        _compare(name, t, v.GetData(), refs_[0][t])


def test_model_inputs_reach_the_products(model_refs):
    """scores, probabilities and context are spread out: a wrong product would show at the output"""
    for name, (buf, xs, refs_) in model_refs.items():
        if name == "attention_f32":
            continue
        for o in read(buf)["ops"]:
            if o["builtin"] == B.BATCH_MATMUL:
                r = refs_[0][o["outputs"][0]].astype(np.int32)
                inside = float(((r > -128) & (r < 127)).mean())
                assert len(np.unique(r)) >= 16 and inside >= 0.5, (name, o["outputs"], len(np.unique(r)), inside)


def test_attention_block_default_registers_whole_on_cpu():
    """the default (tokens 196, dim 192, 3 heads) block and vit_tiny at 224: zero unsupported ops"""
    from band_amd.tflite_synth import attention_block, vit_tiny
    for buf in (attention_block(), vit_tiny()):
        spec = HipModelExecutor(0, 0, DeviceFlag.kCPU).InvestigateModelSpec(_model(buf))
        assert spec.unsupported_ops[DeviceFlag.kCPU] == set()


# ---- job batching --------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["attention_17_48_3", "vit_tiny_32", "const_rhs"])
@pytest.mark.parametrize("n", [2, 3])
def test_job_batches_on_cpu(model_refs, name, n):
    """a batchable model at job batches 2 and 3 against the per-job references"""
    buf, xs, refs_ = model_refs[name]
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(0, 0)
    st = ex.PrepareJobBatches(m, key, 3)
    assert st.ok(), st.message()
    assert ex.MaxJobBatch(key) == 3
    for s in range(n):
        ex.GetJobSlotView(key, ex.GetInputs(key)[0], n, s).GetData()[...] = xs[s]
    assert ex.ExecuteJobBatch(key, n).ok()
    for s in range(n):
        for t in ex.GetOutputs(key):
            _compare("%s n=%d slot %d" % (name, n, s), t,
                     ex.GetJobSlotView(key, t, n, s).GetData().reshape(refs_[s][t].shape), refs_[s][t])


def test_rank2_activation_is_not_batchable_but_runs():
    buf = B.rank2_model()
    m = _model(buf)
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    assert ex.InvestigateModelSpec(m).unsupported_ops[DeviceFlag.kCPU] == set()
    assert ex.PrepareSubgraph(m).ok()
    key = SubgraphKey(0, 0)
    st = ex.PrepareJobBatches(m, key, 3)
    assert not st.ok() and "job batching: BATCH_MATMUL with a rank-2 activation operand" in st.message(), st.message()
    assert ex.MaxJobBatch(key) == 1
    x = R.zoo_input(buf, seed=4)
    ref = run_reference(buf, x)
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = x
    assert ex.ExecuteSubgraph(key).ok()
    t = ex.GetOutputs(key)[0]
    assert len(np.unique(ref[t])) >= 16
    np.testing.assert_array_equal(ex.GetTensorView(key, t).GetData().reshape(ref[t].shape), ref[t])


# ---- the Python reader ----------------------------------------------------------------------
def test_python_reader_reads_the_options():
    assert OPT["BatchMatMulOptions"] in OPTION_FIELDS
    ops = [o for o in read(B.MODELS["attention_17_48_3"]())["ops"] if o["builtin"] == B.BATCH_MATMUL]
    assert len(ops) == 2 and all(o["options_type"] == OPT["BatchMatMulOptions"] for o in ops)
    adj = [[o["options"].fields.get(s, (None, 0))[1] for s in (0, 1, 2)] for o in ops]
    assert adj == [[0, 1, 0], [0, 0, 0]], adj
