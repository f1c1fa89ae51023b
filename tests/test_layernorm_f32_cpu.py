"""The float32 LayerNorm rule judged without a GPU: the numpy restatement of
tests.layernorm_f32_models against the float64 LayerNorm at the bound derived
there, and against its wrong variants; the launcher's parameter check (pure
host); and the switches a host can see - nothing names the fused kernel unless
BAND_HIP_FUSED_LAYERNORM_F32 is set, and the kCPU worker ignores the variable.

Largest |restatement - real| / bound observed over every launcher case and data
kind: 0.24 (9x1023_const).

Bit-wise differences at SEED = 2024: "serial" differs from the rule on 21 of the
36 cases, the first 7x64_normal; "fma" on 27, the first 1x1_normal."""
import ctypes

import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey, _abi
from tests import float_harness as H
from tests import layernorm_f32_models as L

CASES = L.launcher_cases()


def test_launcher_cases_cover_the_issue():
    assert {(c.rows, c.depth) for c in CASES} == {(1, 1), (3, 5), (7, 64), (5, 65), (17, 48), (4, 192), (2, 1000),
                                                  (9, 1023), (1, 1024)}
    assert {c.kind for c in CASES} == {"normal", "cancel", "const", "zeros"}
    assert len(CASES) == 36
    for c in CASES:
        if c.kind == "const":
            assert (c.x == c.x[:, :1]).all()
        if c.kind == "cancel":
            assert np.abs(c.x - 1000).max() < 0.1


def test_restatement_within_the_derived_bound():
    worst, where = 0.0, ""
    for c in CASES:
        bound = c.bound()
        assert np.isfinite(bound).all(), c.name
        ratio = H.check(c.ref(), c.real(), bound, c.name)
        if ratio > worst:
            worst, where = ratio, c.name
    print("layernorm_f32 restatement: largest |got - real| / bound = %.3g (%s)" % (worst, where))
    assert worst < 1.0


def test_rule_sum_is_the_documented_order():
    """64 lane sums of four float4 steps in ascending index order, then the butterfly - spelled out element by element"""
    rng = np.random.default_rng(5)
    for c in (1, 5, 64, 65, 1000, 1024):
        x = (rng.normal(0, 1, c) * 10.0 ** rng.integers(-3, 4, c)).astype(L.F)
        lanes = [L.F(0.0)] * 64
        for j in range(4):
            for lane in range(64):
                for k in range(4):
                    i = 256 * j + 4 * lane + k
                    if i < c:
                        lanes[lane] = L.F(lanes[lane] + x[i])
        for o in (32, 16, 8, 4, 2, 1):
            lanes = [L.F(lanes[lane] + lanes[lane ^ o]) for lane in range(64)]
        assert len({v.tobytes() for v in lanes}) == 1
        assert L.rule_sum(x[None, :])[0].tobytes() == lanes[0].tobytes(), c


@pytest.mark.parametrize("wrong,kind", [("one_pass", "cancel"), ("no_eps", "const"), ("c_minus_1", "normal")])
def test_wrong_variants_exceed_the_bound(wrong, kind):
    n = 0
    for c in CASES:
        if c.kind != kind or (wrong == "c_minus_1" and c.depth == 1):
            continue
        if wrong == "one_pass" and c.depth == 1:
            continue  # E[x^2] - m^2 of one element is exact: fl(x^2) - fl(x^2) = 0
        assert not H.accepts(c.ref(wrong), c.real(), c.bound()), "%s passes as %s" % (wrong, c.name)
        n += 1
    assert n >= 8


@pytest.mark.parametrize("wrong", ["serial", "fma"])
def test_reassociated_and_fused_variants_differ_bitwise(wrong):
    differ = [c.name for c in CASES if c.ref(wrong).tobytes() != c.ref().tobytes()]
    print("layernorm_f32 %s differs bit-wise on %d of %d cases, first %s" % (wrong, len(differ), len(CASES),
                                                                            differ[:1]))
    assert differ, wrong
    # and both stay inside the bound: they are other roundings of the same LayerNorm, not other functions
    for c in CASES:
        if c.name == differ[0]:
            H.check(c.ref(wrong), c.real(), c.bound(), "%s %s" % (wrong, c.name))


def test_nonfinite_case_has_nan_at_known_positions():
    c = L.LnCase(*L.NONFINITE_SHAPE, "nonfinite")
    y = c.ref()
    assert np.isfinite(y[0]).all() and np.isfinite(y[4]).all()
    assert np.isnan(y[1:4]).all()


# ---- the launcher's check (pure host) ----------------------------------------------------
PTR = 1 << 20  # never dereferenced


def test_check_accepts_every_launcher_case():
    lib = _abi.load()
    for rows, depth in L.SHAPES:
        for mode in L.MODES:
            p = L.params(rows, depth)
            p.input = p.gamma = p.beta = PTR
            if mode == "out" or mode.startswith("both"):
                p.output = PTR
            if mode != "out":
                p.q = p.scale = p.offset = PTR
            assert lib.bh_layernorm_f32_check(ctypes.byref(p)) == 0, lib.bh_last_error()
            assert lib.bh_layernorm_f32_kernel(ctypes.byref(p)) == L.KERNEL.encode()


@pytest.mark.parametrize("name,change,reason", L.REFUSALS, ids=[r[0] for r in L.REFUSALS])
def test_check_refuses_by_name(name, change, reason):
    lib = _abi.load()
    p = L.valid_block(PTR)
    assert lib.bh_layernorm_f32_check(ctypes.byref(p)) == 0, lib.bh_last_error()
    assert lib.bh_layernorm_f32_kernel(ctypes.byref(p)) == L.KERNEL.encode()
    for k, v in change.items():
        setattr(p, k, v)
    assert lib.bh_layernorm_f32_check(ctypes.byref(p)) != 0, name
    msg = lib.bh_last_error().decode()
    assert msg.startswith("bh_layernorm_f32: ") and reason in msg, msg
    assert lib.bh_layernorm_f32_kernel(ctypes.byref(p)) == b"", name
    assert lib.bh_layernorm_f32_check(None) != 0 and lib.bh_layernorm_f32_kernel(None) == b""


def test_abi_mirror_matches_the_header_layout():
    """long, int, float, seven pointers, int (padded to the pointers' alignment)"""
    assert ctypes.sizeof(_abi.LayerNormF32Params) == 8 + 4 + 4 + 7 * 8 + 8
    assert _abi.LayerNormF32Params.input.offset == 16 and _abi.LayerNormF32Params.asymmetric.offset == 72
    assert _abi.LAYERNORM_F32_MAX_DEPTH == L.MAX_DEPTH


# ---- the switches, as far as a host sees them ----------------------------------------------
def _cpu_kernels(buf):
    m = HipModel(0)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(0, 0, DeviceFlag.kCPU)
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    return ex.LaunchKernels(SubgraphKey(0, 0))


def test_cpu_worker_ignores_the_variable(monkeypatch):
    buf = L.ln_qkv("asymmetric")
    monkeypatch.delenv(L.FLAG, raising=False)
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    plain = _cpu_kernels(buf)
    assert not any("layernorm_f32" in k for k in plain), plain
    assert len(plain) == 10 + 2 * 3 and plain.count("dynquant_rows_host") == 3, plain
    monkeypatch.setenv(L.FLAG, "1")
    assert _cpu_kernels(buf) == plain


def test_cpu_worker_runs_the_ten_host_kernels_with_the_variable_set(monkeypatch):
    """and its result stays within the ops' bounds (tests.float_harness.check_graph_ops)"""
    from tests import hybrid_models as Y
    monkeypatch.setenv(L.FLAG, "1")
    buf = L.ln_qkv("symmetric")
    om, runs = H.run_executor(buf, [Y.model_feed(buf, seed=3)], DeviceFlag.kCPU, 0, view_all=True)
    assert H.check_graph_ops(om, runs[0], "ln_qkv kCPU")[1]["fc"] == 3
