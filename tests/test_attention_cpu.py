"""The fused attention launch without a GPU: the composed reference of
tests.attention_models against run_reference on a model, the case set's
coverage, every refusal of bh_attention_i8_check with its reason, the LDS a
launch takes, the directed properties of the reference (clamped scores, flat
rows, an underflowing table, the sum-order case) and the kCPU executor, which
ignores BAND_HIP_FUSED_ATTENTION."""
import ctypes

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi
from oracle import runner as orc
from oracle.tflite_fb import Model as OModel
from tests import attention_models as A
from tests import bmm_models as B
from tests import encoder_models as E
from tests import reindex_models as R
from tests.graph_reference import run_reference

CASES = A.launcher_cases()


def test_composed_reference_equals_run_with_bmm_on_a_model():
    """scores / probabilities / context of attention_block(17, 48, 3) taken from run_reference's q, k, v through
    AttnCase's three steps"""
    buf = A.MODELS["attention_17_48_3"]()
    om = OModel(buf)
    vals = run_reference(buf, R.zoo_input(buf, seed=3))
    (sc, pr, ctx), = A.attention_tensors(buf)
    first = next(o for o in om.operators if o.outputs[0] == sc)
    second = next(o for o in om.operators if o.outputs[0] == ctx)
    tq, tk, tv = first.inputs[0], first.inputs[1], second.inputs[1]
    q = lambda t: (float(om.tensors[t].scale[0]), int(om.tensors[t].zero_point[0]))
    c = A.AttnCase("model", (1, 3), 17, 17, 16, 16, zps=(q(tq)[1], q(tk)[1], q(sc)[1]),
                   qk_scales=(q(tq)[0], q(tk)[0], q(sc)[0]), v_zp=q(tv)[1], out_zp=q(ctx)[1],
                   pv_scales=(q(pr)[0], q(tv)[0], q(ctx)[0]))
    assert q(pr) == (1.0 / 256, -128)
    c.q, c.k, c.v = vals[tq], vals[tk], vals[tv]
    np.testing.assert_array_equal(c.scores(), vals[sc])
    np.testing.assert_array_equal(c.probs(), vals[pr])
    np.testing.assert_array_equal(c.ref(), vals[ctx])


def test_case_set_covers_the_issues_values():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    for vals, attr in ((A.ROWS, "rows"), (A.KEYS, "keys"), (A.HEAD_DIMS, "head_dim"), (A.OUT_DIMS, "out_dim")):
        assert set(vals) <= {getattr(c, attr) for c in CASES}, attr
    assert {(1, 1), (2, 3), (1, 5)} <= {c.batch for c in CASES}
    assert {"dense", "heads"} == {c.layout for c in CASES}
    for which in range(4):
        assert {1, 4} <= {c.misalign[which] for c in CASES}
    lib = _abi.load()
    fast = set()
    for c in CASES:
        for m, s, k in ((c.qk_mult, c.qk_shift, c.head_dim), (c.pv_mult, c.pv_shift, c.keys)):
            mm, ss = ctypes.c_int32(m), ctypes.c_int32(s)
            fast.add(lib.bh_conv_requant_fast_ok(ctypes.byref(mm), ctypes.byref(ss), 1, k, 0))
    assert fast == {0, 1}
    assert next(c for c in CASES if c.name == "qk_left_shift").qk_shift > 0
    assert next(c for c in CASES if c.name == "pv_left_shift").pv_shift > 0
    assert {0} < {c.z_v for c in CASES}


@pytest.mark.parametrize("name,change,reason", A.refused_params(), ids=[r[0] for r in A.refused_params()])
def test_parameter_checks_say_why(name, change, reason):
    from band_amd import backend  # noqa: F401
    lib = _abi.load()
    p, bufs, _ = A.prepare(A.valid_case(), device=False)
    assert lib.bh_attention_i8_check(ctypes.byref(p)) == 0, lib.bh_last_error()
    assert lib.bh_attention_i8_kernel(ctypes.byref(p)) == A.KERNEL.encode()
    assert lib.bh_attention_i8_lds_bytes(ctypes.byref(p)) > 0
    change(p)
    assert lib.bh_attention_i8_check(ctypes.byref(p)) != 0
    msg = lib.bh_last_error().decode()
    assert msg.startswith("bh_attention_i8: ") and reason in msg, msg
    assert lib.bh_attention_i8_kernel(ctypes.byref(p)) == b""
    assert lib.bh_attention_i8_lds_bytes(ctypes.byref(p)) == 0
    assert lib.bh_attention_i8_check(None) != 0 and "null parameter block" in lib.bh_last_error().decode()


def test_lds_of_a_launch():
    """64 x (roundup(keys, 64) + 16) of strip, 128 x 80 of V staging, 1 KB of table; the largest fits a CU's 160 KiB"""
    lib = _abi.load()
    p, bufs, _ = A.prepare(A.valid_case(), device=False)
    for keys, strip in ((1, 64 * 80), (64, 64 * 80), (65, 64 * 144), (196, 64 * 272), (1024, 64 * 1040)):
        p.keys = keys
        assert lib.bh_attention_i8_lds_bytes(ctypes.byref(p)) == strip + 128 * 80 + 1024
        assert ((keys + 63) // 64 * 64 + 16) // 16 % 2 == 1  # an odd number of 16-byte slots per row
    assert 64 * 1040 + 128 * 80 + 1024 <= 160 * 1024
    assert _abi.ATTENTION_MAX_KEYS == 1024 and _abi.ATTENTION_MAX_DIM == 128


# ---- directed properties, asserted on the reference alone -----------------------------------
def test_clamp_case_saturates_at_both_bounds():
    s = A.clamp_case().scores()
    lo, hi = (s == -128).mean(), (s == 127).mean()
    print("clamps: %.1f %% at -128, %.1f %% at 127" % (100 * lo, 100 * hi))
    assert lo >= 0.05 and hi >= 0.05 and 1 - lo - hi >= 0.25


def test_flat_rows_have_equal_probabilities():
    c = A.flat_case()
    s, p = c.scores(), c.probs()
    assert (s == c.z_s).all()
    assert (p == p[..., :1]).all() and (p > -128).all()


def test_peak_cases_put_the_maximum_where_they_say():
    for first in (True, False):
        c = A.peak_case(first)
        s = c.scores()
        at = 0 if first else -1
        assert (s.argmax(-1) == (0 if first else c.keys - 1)).all()
        assert (s[..., at] > np.delete(s, at % c.keys, axis=-1).max(-1)).all()
        assert (c.probs()[..., at] == 127).all()


def test_underflow_case_gathers_zeros():
    c = next(c for c in CASES if c.name == "table_underflows")
    t = orc.softmax_table(c.in_scale, 1.0)
    assert t[0] == 0.0 and t[255] == 1.0
    s = c.scores().astype(np.int32)
    e = t[255 - s.max(-1, keepdims=True) + s]
    print("underflow: %.1f %% of the gathers are 0" % (100 * (e == 0).mean()))
    assert (e == 0).mean() > 0.5 and ((e == 0).sum(-1) > c.keys // 2).all()


def test_np_softmax_in_order_is_the_oracles():
    for name in ("ext_65x65x128x1", "clamps", "table_underflows", "batch_2x3_dense"):
        c = next(c for c in CASES if c.name == name)
        s = c.scores()
        np.testing.assert_array_equal(A.np_softmax(s, c.in_scale), c.probs(s), err_msg=name)


def test_sum_order_case_tells_the_orders_apart():
    """Reversing the row sum, or taking it pairwise, changes at least one probability byte in at least
    SUM_ORDER_FLOOR = 32 rows each of the directed case.  Random rows do not give this (786,432 random q rows against
    a random K gave 15 rows for the reversed sum and 11 for the pairwise one, in 14 s), so
    tests.attention_models.sum_order_case directs its seeded candidates at rounding ties of the largest probability
    and keeps the rows that differ: 3,000 candidates, about a second, 32 rows kept for each order.  Asserted against
    the oracle's softmax on the oracle's scores."""
    case, rev_rows, pair_rows = A.sum_order()
    s = case.scores()[0, 0]
    ref = case.probs()[0, 0]
    np.testing.assert_array_equal(A.np_softmax(s, case.in_scale), ref)
    rev = (A.np_softmax(s, case.in_scale, "reversed") != ref).any(-1)
    pair = (A.np_softmax(s, case.in_scale, "pairwise") != ref).any(-1)
    print("sum order: %d rows differ reversed, %d pairwise, of %d" % (rev.sum(), pair.sum(), case.rows))
    assert case.keys == 196
    assert rev[rev_rows].all() and pair[pair_rows].all()
    assert len(rev_rows) >= A.SUM_ORDER_FLOOR and len(pair_rows) >= A.SUM_ORDER_FLOOR
    # and the difference survives P V: the context bytes change too in some of those rows
    def ctx(order):
        p = A.np_softmax(s, case.in_scale, order)[None, None]
        return B.bmm_eval(p, case.v, False, False, case.z_p, case.z_v, case.z_o, case.pv_mult, case.pv_shift)
    np.testing.assert_array_equal(ctx("forward"), case.ref())
    print("sum order: context rows that differ: reversed %d, pairwise %d" % (
        (ctx("reversed") != case.ref()).any(-1).sum(), (ctx("pairwise") != case.ref()).any(-1).sum()))


# ---- the kCPU executor ignores the flag -------------------------------------------------------
def test_cpu_executor_ignores_the_flag(monkeypatch):
    from band_amd import backend  # noqa: F401
    monkeypatch.setenv("BAND_HIP_FUSED_ATTENTION", "1")
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    buf = A.MODELS["attention_17_48_3"]()
    x = E.model_input(buf, seed=5)
    ref = run_reference(buf, x)
    m = HipModel(0)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, 0)
    kernels = ex.LaunchKernels(key)
    assert A.KERNEL not in kernels and kernels.count("batch_matmul_host") == 2, kernels
    ex.GetTensorView(key, ex.GetInputs(key)[0]).GetData()[...] = x
    assert ex.ExecuteSubgraph(key).ok()
    for t in ex.GetOutputs(key):
        np.testing.assert_array_equal(ex.GetTensorView(key, t).GetData().reshape(ref[t].shape), ref[t])
