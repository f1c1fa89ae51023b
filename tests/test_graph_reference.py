"""The shared reference code of the tests, judged alone: tests.fixed_point
against the oracle's C code on directed_harness's grid, the sensitivity of
that grid to each mutant, the disjoint claims of tests.graph_reference's table
on every family model, and one model that needs evaluators of three families
at once, on both workers."""
import numpy as np
import pytest

from band_amd import DeviceFlag, HipModel, HipModelExecutor, SubgraphKey
from band_amd.tflite_synth import QGraph
from oracle import runner as orc
from oracle.tflite_fb import Model as OModel
from tests import attention_models as A
from tests import bmm_models as B
from tests import directed_harness as dh
from tests import encoder_models as E
from tests import fixed_point as fp
from tests import graph_reference as GR
from tests import grouped_models as G
from tests import reindex_models as R

INT32_MAX = (1 << 31) - 1


# ---- fixed point ------------------------------------------------------------------------
def _grid():
    """[(mult, shift, accumulators)]: MULTS x (-e for ES, +left for LEFTS); per pair 0, +-1, the largest
    accumulators the left shift does not overflow, and a positive and a negative step-2 tie where e > 0"""
    out = []
    for m in dh.MULTS:
        for shift in [-e for e in dh.ES] + list(dh.LEFTS):
            top = INT32_MAX >> max(shift, 0)
            accs = [0, 1, -1, top, -top, top - 1, 1 - top, 12345, -12345]
            accs += [dh.tie_acc(m, -shift, sign) for sign in (1, -1) if shift < 0]
            out.append((m, shift, accs))
    return out


GRID = _grid()


def test_grid_holds_both_rounding_ties():
    for m, shift, accs in GRID:
        pos, neg = dh.ties(np.array(accs), m, shift)
        assert (pos.any() and neg.any()) == (shift < 0), (m, shift)


def test_mbqm_equals_the_oracle_scalar_and_array():
    tfl_mbqm = orc.lib().tfl_mbqm
    n = 0
    for m, shift, accs in GRID:
        want = [tfl_mbqm(a, m, shift) for a in accs]
        got = [fp.mbqm(a, m, shift) for a in accs]
        assert all(isinstance(v, int) for v in got)
        assert got == want, (m, shift)
        np.testing.assert_array_equal(fp.mbqm(np.array(accs, np.int64), m, shift), want, err_msg=str((m, shift)))
        n += len(accs)
    assert n > 500
    # per-channel mult / shift on the last axis: column c is pair c of the grid, row r its accumulator r
    # (the first nine accumulators exist for every pair)
    acc = np.array([accs[:9] for _, _, accs in GRID], np.int64).T
    mult = np.array([m for m, _, _ in GRID], np.int64)
    shift = np.array([s for _, s, _ in GRID], np.int32)
    want = np.array([[tfl_mbqm(int(a), int(m), int(s)) for a, m, s in zip(row, mult, shift)] for row in acc])
    np.testing.assert_array_equal(fp.mbqm(acc, mult, shift), want)


def test_python_ints_beyond_int64():
    """the scalar path is arbitrary precision: 2^70 x 2^30 / 2^31 = 2^69, and a tie of e = 40 rounds away from zero"""
    assert fp.srdhm(1 << 70, 1 << 30) == 1 << 69
    assert fp.rdbypot(-(3 << 39), 40) == -2 and fp.rdbypot(3 << 39, 40) == 2
    assert fp.sat_shl(1 << 28, 3) == INT32_MAX and fp.sat_shl(-(1 << 28), 3) == -(1 << 31) and fp.sat_shl(5, 3) == 40


@pytest.mark.parametrize("mutant", dh.MUTANTS)
def test_every_mutant_shows_on_the_grid(mutant):
    """the epilogue of directed_harness (zero point 3, the full int8 window: ties of both signs stay inside it)
    on the grid's accumulators"""
    differs = 0
    for m, shift, accs in GRID:
        acc = np.array(accs, np.int64)
        good = dh.epilogue_np(acc, m, shift, 3, -128, 127, np.int8)
        differs += int((dh.epilogue_np(acc, m, shift, 3, -128, 127, np.int8, mutant) != good).sum())
    assert differs > 0, mutant


def test_round_half_away_both_widths():
    v = np.array([0.5, -0.5, 1.5, -1.5, 2.4999998, -2.4999998, 0.0, 8388609.0], np.float32)
    np.testing.assert_array_equal(fp.round_half_away(v), np.array([1, -1, 2, -2, 2, -2, 0, 8388609], np.float32))
    assert [fp.round_half_away64(float(x)) for x in v[:4]] == [1.0, -1.0, 2.0, -2.0]


# ---- the walker's claims ------------------------------------------------------------------
def _family_models():
    out = {"reindex/" + k: b for k, b in R.ZOO.items()}
    out.update({"bmm/" + k: b for k, b in B.MODELS.items()})
    out.update({"encoder/" + k: b for k, b in E.MODELS.items()})
    out.update({"attention/" + k: b for k, b in A.MODELS.items()})
    out.update({"grouped/" + b.__name__: b for b in (G.conv_then_add, G.conv_then_relu6, G.shufflenet_small)})
    out["reindex/batch_axis_transpose"] = R.batch_axis_transpose
    out["bmm/rank2"] = B.rank2_model
    return out


FAMILY_MODELS = _family_models()


@pytest.mark.parametrize("name", sorted(FAMILY_MODELS))
def test_claims_are_disjoint_on_family_models(name):
    om = OModel(FAMILY_MODELS[name]())
    claimed = [GR.claimants(om, o) for o in om.operators]
    assert all(len(c) <= 1 for c in claimed), claimed
    assert any(claimed), "a family model without an op of its family"


def mixed_model():
    """grouped CONV_2D (2 groups, 3x3, on [1, 4, 4, 8], 5 channels per group) -> RESHAPE to 16 rows of 10 ->
    last-axis MEAN, SQUARED_DIFFERENCE with it, and BATCH_MATMUL of the rows with themselves: evaluators of
    grouped_models, encoder_models and bmm_models in one graph, the rest the oracle's"""
    g = QGraph(np.int8, seed=97, name="grouped_mean_bmm")
    x = g.input([1, 4, 4, 8], scale=0.05)
    y = g.reshape(g.conv(x, 10, k=3, act="NONE", groups=2), [1, 16, 10])
    s = g.meta[y][1]
    m = g.mean_last(y)
    g.output(g.squared_difference(y, m, (128 * s) ** 2 / 255.0, -128))
    g.output(g.batch_matmul(y, y, adj_y=True))
    return g.build()


def test_an_overlapping_entry_makes_the_walker_raise():
    buf = mixed_model()
    x = R.zoo_input(buf, seed=1)
    GR.run_reference(buf, x, GR.TABLE)
    overlapping = [GR.TABLE[0], (lambda om, o: o.builtin == G.CONV_2D, G.eval_grouped)] + GR.TABLE[1:]
    with pytest.raises(AssertionError, match="claimed by entries"):
        GR.run_reference(buf, x, overlapping)


@pytest.fixture(scope="module")
def mixed_refs():
    buf = mixed_model()
    om = OModel(buf)
    assert [GR.claimants(om, o) for o in om.operators] == [[0], [], [3], [3], [2]]
    xs = [R.zoo_input(buf, seed=80 + i) for i in range(3)]
    refs = [GR.run_reference(buf, x) for x in xs]
    for ref in refs:  # no output is constant or saturated throughout
        for t in om.outputs:
            assert len(np.unique(ref[t])) >= 16, t
    return buf, om, xs, refs


def _run_mixed(mixed_refs, flag, worker):
    buf, om, xs, refs = mixed_refs
    m = HipModel(0)
    assert m.FromBuffer(buf).ok()
    ex = HipModelExecutor(0, worker, flag)
    assert ex.InvestigateModelSpec(m).unsupported_ops[flag] == set()
    st = ex.PrepareSubgraph(m)
    assert st.ok(), st.message()
    key = SubgraphKey(0, worker)
    watch = [t.index for t in om.tensors if not t.is_const]
    views = {t: ex.GetTensorView(key, t) for t in watch}
    for x, ref in zip(xs, refs):  # on the GPU worker: eager, capture, replay
        ex.GetTensorView(key, om.inputs[0]).GetData()[...] = x
        assert ex.ExecuteSubgraph(key).ok()
        for t, v in views.items():
            np.testing.assert_array_equal(v.GetData().reshape(ref[t].shape), ref[t], err_msg="tensor %d" % t)


def test_mixed_family_model_on_cpu_worker(mixed_refs):
    _run_mixed(mixed_refs, DeviceFlag.kCPU, 0)


@pytest.mark.gpu
def test_mixed_family_model_on_gpu_worker(gpu_lib, monkeypatch, mixed_refs):
    monkeypatch.delenv("BAND_HIP_FUSION", raising=False)
    _run_mixed(mixed_refs, DeviceFlag.kGPU, 1)
