"""Fixtures of BATCH_MATMUL (int8 / float32): the cases, the references, the
launcher parameter blocks (host or device buffers), the models and eval_bmm
(one operator for tests.graph_reference).

int8 reference: the oracle's FULLY_CONNECTED (its C code, unchanged) per batch
slice, `orc.fully_connected(lhs[b], rhs[b]^T, None, in_zp=z_l, w_zp=z_r,
out_zp=z_o, mult, shift, amin=-128, amax=127)` with `orc.quantize_multiplier`
for the pair; slices that share an rhs slice are stacked into one call (the
arithmetic is per row).  float32 reference: the float64 product with the bound
gamma(K + 2) sum|a||b| + 2^-126 (tests/float_harness.py).  An expected value
never comes from the product.

np_bmm is an independent numpy restatement of the int8 formula; the CPU test
first shows it equal to bmm_ref and then uses its `wrong=` variants to show
that the cases tell each mistake apart."""
import ctypes

import numpy as np

from band_amd.tflite_synth import QGraph, attention_block, vit_tiny
from oracle import runner as orc
from tests import float_harness as H
from tests.fixed_point import rdbypot
from tests.grouped_models import SLACK, _buffer

BATCH_MATMUL = 126
KERNEL = "bmm_mfma_kernel"


# ---- cases ---------------------------------------------------------------------
class BmmCase:
    """lhs / rhs as stored (adj_x: [.., K, M]; adj_y: [.., N, K]); int8 cases
    carry zero points and the (mult, shift) pair of their three scales"""

    def __init__(self, name, lhs_shape, rhs_shape, adj_x=False, adj_y=False, zps=(3, -5, 7), scales=(0.02, 0.03, 0.05),
                 spread=None, seed=0, dtype=np.int8, fill=None, misalign=(0, 0), hint=0):
        self.name, self.adj_x, self.adj_y, self.dtype = name, adj_x, adj_y, np.dtype(dtype)
        self.misalign, self.hint = misalign, hint
        rng = np.random.default_rng(seed)
        self.z_l, self.z_r, self.z_o = zps
        if self.dtype == np.int8:
            def draw(shape, zp, which):
                if fill is not None:
                    return np.full(shape, fill[which], np.int8)
                if spread is None:
                    return rng.integers(-128, 128, shape).astype(np.int8)
                return np.clip(zp + rng.integers(-spread, spread + 1, shape), -128, 127).astype(np.int8)
            self.lhs, self.rhs = draw(lhs_shape, self.z_l, 0), draw(rhs_shape, self.z_r, 1)
        else:
            self.lhs = rng.uniform(-1, 1, lhs_shape).astype(np.float32)
            self.rhs = rng.uniform(-1, 1, rhs_shape).astype(np.float32)
        self.scales = scales
        if self.dtype == np.int8:
            s_l, s_r, s_o = scales
            # FullyConnectedMultiplier: the float32 product of the input scales over the output scale, in double
            self.mult, self.shift = orc.quantize_multiplier(float(np.float32(s_l) * np.float32(s_r)) / float(np.float32(s_o)))

    def views(self, lhs=None, rhs=None):
        """(A [b0, b1, M, K], B [b0, b1, K, N]) broadcast views of the stored operands"""
        a = self.lhs if lhs is None else lhs
        b = self.rhs if rhs is None else rhs
        a = np.swapaxes(a, -1, -2) if self.adj_x else a
        b = np.swapaxes(b, -1, -2) if self.adj_y else b
        lead = np.broadcast_shapes(a.shape[:-2], b.shape[:-2])
        lead = (1,) * (2 - len(lead)) + tuple(lead)
        a = np.broadcast_to(a, lead + a.shape[-2:])
        b = np.broadcast_to(b, lead + b.shape[-2:])
        assert a.shape[-1] == b.shape[-2]
        return a, b

    @property
    def mnk(self):
        a, b = self.views()
        return a.shape[-2], b.shape[-1], a.shape[-1]

    @property
    def out_shape(self):
        a, b = self.views()
        lead = np.broadcast_shapes(self.lhs.shape[:-2], self.rhs.shape[:-2])
        return tuple(lead) + (a.shape[-2], b.shape[-1])


def fc_slices(A, B, rhs_lead, call):
    """out [b0, b1, M, N] of broadcast views A, B: one `call(rows [n M, K], w [N, K])`
    per distinct rhs slice (rhs_lead: the rhs's own leading dims padded to 2)"""
    b0, b1, M, K = A.shape
    N = B.shape[-1]
    out = None
    for r0 in range(rhs_lead[0]):
        for r1 in range(rhs_lead[1]):
            s0 = slice(None) if rhs_lead[0] == 1 and b0 > 1 else slice(r0, r0 + 1)
            s1 = slice(None) if rhs_lead[1] == 1 and b1 > 1 else slice(r1, r1 + 1)
            rows = np.ascontiguousarray(A[s0, s1]).reshape(-1, K)
            w = np.ascontiguousarray(B[s0, s1][0, 0].T)
            y = call(rows, w)
            if out is None:
                out = np.zeros((b0, b1, M, N), y.dtype)
            out[s0, s1] = y.reshape(out[s0, s1].shape)
    return out


def _rhs_lead(shape):
    """the rhs's own leading dims, padded to two"""
    lead = tuple(shape[:-2])
    return (1,) * (2 - len(lead)) + lead


def bmm_eval(lhs, rhs, adj_x, adj_y, z_l, z_r, z_o, mult, shift):
    """int8 BATCH_MATMUL through the oracle's FULLY_CONNECTED per rhs slice"""
    a = np.swapaxes(lhs, -1, -2) if adj_x else lhs
    b = np.swapaxes(rhs, -1, -2) if adj_y else rhs
    lead = np.broadcast_shapes(a.shape[:-2], b.shape[:-2])
    lead2 = (1,) * (2 - len(lead)) + tuple(lead)
    A = np.broadcast_to(a, lead2 + a.shape[-2:])
    B = np.broadcast_to(b, lead2 + b.shape[-2:])

    def call(rows, w):
        return orc.fully_connected(rows, w, None, in_zp=z_l, w_zp=z_r, out_zp=z_o, mult=mult, shift=shift,
                                   amin=-128, amax=127)
    out = fc_slices(A, B, _rhs_lead(rhs.shape), call)
    return out.reshape(tuple(lead) + out.shape[-2:])


def bmm_ref(case):
    """the expected output: int8 exactly; float32 as (float64 product, bound)"""
    if case.dtype == np.int8:
        return bmm_eval(case.lhs, case.rhs, case.adj_x, case.adj_y, case.z_l, case.z_r, case.z_o, case.mult,
                        case.shift)
    A, B = case.views()
    with np.errstate(invalid="ignore", over="ignore"):
        ref = np.matmul(A.astype(np.float64), B.astype(np.float64))
        mag = np.matmul(np.abs(A).astype(np.float64), np.abs(B).astype(np.float64))
    K = A.shape[-1]
    return ref.reshape(case.out_shape), (H.gamma(K + 2) * mag + H.FLOOR).reshape(case.out_shape)


# ---- an independent numpy restatement, with the mistakes a kernel can make -----
def step1(case):
    """(int64 accumulators, the value after step 1) of the case"""
    A, B = case.views()
    acc = np.matmul(A.astype(np.int64) - case.z_l, B.astype(np.int64) - case.z_r)
    x = acc << max(case.shift, 0)
    return acc, (x * int(case.mult) + (1 << 30)) >> 31


def np_bmm(case, wrong=None):
    """the folded form sum ab - z_r sum_k a - z_l sum_k b + K z_l z_r, requantised;
    wrong in (None, "adj_y", "no_colsum", "no_kzz", "padded_k", "slice0", "half_up")"""
    lhs, rhs = case.lhs, case.rhs
    if wrong == "slice0":
        rhs = np.broadcast_to(rhs.reshape((-1,) + rhs.shape[-2:])[0], rhs.shape)
    if wrong == "adj_y":
        b = rhs if case.adj_y else np.swapaxes(rhs, -1, -2)  # the other reading of the same bytes
        a = np.swapaxes(lhs, -1, -2) if case.adj_x else lhs
        lead = np.broadcast_shapes(a.shape[:-2], b.shape[:-2])
        lead2 = (1,) * (2 - len(lead)) + tuple(lead)
        A, B = np.broadcast_to(a, lead2 + a.shape[-2:]), np.broadcast_to(b, lead2 + b.shape[-2:])
    else:
        A, B = case.views(lhs, rhs)
    A, B = A.astype(np.int64), B.astype(np.int64)
    K = A.shape[-1]
    acc = np.matmul(A, B) - case.z_r * A.sum(-1, keepdims=True)
    if wrong != "no_colsum":
        acc = acc - case.z_l * B.sum(-2, keepdims=True)
    if wrong != "no_kzz":
        acc = acc + (-(-K // 64) * 64 if wrong == "padded_k" else K) * case.z_l * case.z_r
    y = ((acc << max(case.shift, 0)) * int(case.mult) + (1 << 30)) >> 31
    v = rdbypot(y, max(-case.shift, 0), mutant=wrong) + case.z_o
    return np.clip(v, -128, 127).astype(np.int8).reshape(case.out_shape)


# ---- the launcher cases ----------------------------------------------------------
MS, NS, KS = (1, 15, 16, 17, 33), (1, 15, 16, 17, 65), (1, 15, 16, 63, 64, 65, 130)


def covering_triples():
    """35 (M, N, K): every (M, N), every (M, K) and 31 of the 35 (N, K) pairs of the issue's values"""
    return [(MS[i % 5], NS[(i + i // 5) % 5], KS[i % 7]) for i in range(35)]


def tie_cases():
    """mult = 2^30, shift = -3 (0.5 x 0.25 / 2.0 = 2^-4); inputs within +-3 of their zero points"""
    return [BmmCase("ties_k%d" % k, (17, k), (k, 33), zps=(3, -2, 1), scales=(0.5, 0.25, 2.0), spread=3, seed=400 + k)
            for k in (16, 33)]


def negative_tie_case():
    """mult = 2^30, shift = -3 again, built so that half of the outputs are NEGATIVE step-2 ties: row i of
    lhs - z_l holds one odd r_i, every row k of rhs - z_r holds v_j, so acc = r_i v_j; v_j = -8 on the even
    columns gives step 1 = -4 r_i = 4 (mod 8), a tie below zero (a half-up step 2 lands one higher there)"""
    c = BmmCase("negative_ties", (17, 16), (16, 34), zps=(3, -2, 1), scales=(0.5, 0.25, 2.0), spread=0, seed=0)
    a = np.zeros((17, 16), np.int64)
    a[np.arange(17), np.arange(17) % 16] = 2 * np.arange(17) + 1
    v = np.where(np.arange(34) % 2 == 0, -8, np.array([8, 3, -5, 6, 7, -3, 5])[np.arange(34) % 7])
    c.lhs = (a + c.z_l).astype(np.int8)
    c.rhs = (np.broadcast_to(v, (16, 34)) + c.z_r).astype(np.int8)
    return c


def left_shift_case():
    """0.5 x 0.5 / 0.1 = 2.5: shift +2; small-range inputs keep the output inside the clamp"""
    return BmmCase("left_shift", (17, 33), (33, 33), zps=(2, -1, -3), scales=(0.5, 0.5, 0.1), spread=1, seed=410)


def clamp_case():
    """K = 65 at 0.02 x 0.03 / 0.05 with inputs within +-56 of their zero points: 10.7 % of the reference at
    -128, 14.1 % at 127, 75 % inside (full-range inputs clamp 78 %; +-48 leaves 4.5 % at the low end)"""
    return BmmCase("clamps", (33, 65), (65, 17), zps=(5, -7, 2), scales=(0.02, 0.03, 0.05), spread=56, seed=420)


def launcher_cases():
    cases = []
    for i, (m, n, k) in enumerate(covering_triples()):
        # adj_y alternates, so both the direct and the staged rhs path see every K class
        cases.append(BmmCase("mnk_%dx%dx%d" % (m, n, k), (m, k), (n, k) if i % 2 else (k, n), adj_y=bool(i % 2),
                             spread=40, seed=100 + i))
    for ax in (False, True):
        for ay in (False, True):
            cases.append(BmmCase("adj_%d%d" % (ax, ay), (33, 17) if ax else (17, 33), (65, 33) if ay else (33, 65),
                                 adj_x=ax, adj_y=ay, spread=40, seed=200 + 2 * ax + ay))
    m, k, n = 17, 33, 19
    for name, ls, rs in (("bcast_rhs_lead1", (2, 3, m, k), (1, 3, k, n)), ("bcast_rhs_rank3", (2, 3, m, k), (3, k, n)),
                         ("bcast_lhs_mid1", (2, 1, m, k), (2, 3, k, n)), ("rank2_rank2", (m, k), (k, n)),
                         ("rank2_rhs_under_rank4", (2, 3, m, k), (k, n))):
        for ay in (False, True):
            rs_ = rs[:-2] + (n, k) if ay else rs
            cases.append(BmmCase("%s_adjy%d" % (name, ay), ls, rs_, adj_y=ay, spread=40, seed=300 + len(cases)))
    for zl, zr, fl, fr in ((-128, 127, 127, -128), (127, -128, -128, 127), (0, 0, 127, -128), (-128, 127, -128, 127)):
        for ay in (False, True):
            cases.append(BmmCase("extreme_z%d_%d_a%d_b%d_adjy%d" % (zl, zr, fl, fr, ay), (17, 130),
                                 (16, 130) if ay else (130, 16), adj_y=ay, zps=(zl, zr, 0),
                                 scales=(0.01, 0.01, 0.01 * 0.01 * 130 * 255 * 255 / 120.0), fill=(fl, fr)))
    for which, off in ((0, 1), (0, 4), (1, 1), (1, 4)):
        for ay in (False, True):
            mis = (off, 0) if which == 0 else (0, off)
            cases.append(BmmCase("misaligned_%s%d_adjy%d" % ("lr"[which], off, ay), (17, 64), (32, 64) if ay else (64, 32),
                                 adj_y=ay, spread=40, seed=500 + off + which, misalign=mis))
    # 16-byte units with a K tail, and the same through 1-byte units by hint
    cases.append(BmmCase("vec16_tail", (17, 80), (33, 80), adj_y=True, spread=40, seed=520))
    cases.append(BmmCase("bytes_hint", (17, 80), (33, 80), adj_y=True, spread=40, seed=521, hint=1))
    # one and four 16-column tiles per wave, pinned by hint: N of 1 / 2 / 5 tiles, every adjoint, a K tail,
    # a broadcast rhs, zero points at both ends; then a grid large enough that the launcher routes four by itself
    for hint, tag in ((2, "nt1"), (4, "nt4")):
        for ax in (False, True):
            for ay in (False, True):
                cases.append(BmmCase("%s_adj_%d%d" % (tag, ax, ay), (33, 17) if ax else (17, 33),
                                     (65, 33) if ay else (33, 65), adj_x=ax, adj_y=ay, spread=40, seed=540 + 2 * ax + ay,
                                     hint=hint))
        for ay in (False, True):
            for m, n, k in ((33, 65, 130), (16, 17, 64), (15, 1, 65), (70, 80, 16)):
                cases.append(BmmCase("%s_%dx%dx%d_adjy%d" % (tag, m, n, k, ay), (m, k), (n, k) if ay else (k, n), adj_y=ay,
                                     spread=40, seed=550 + m + ay, hint=hint))
            cases.append(BmmCase("%s_bcast_rhs_rank3_adjy%d" % (tag, ay), (2, 3, 17, 33), (3, 19, 33) if ay else (3, 33, 19),
                                 adj_y=ay, spread=40, seed=560 + ay, hint=hint))
            cases.append(BmmCase("%s_extreme_adjy%d" % (tag, ay), (17, 130), (40, 130) if ay else (130, 40), adj_y=ay,
                                 zps=(-128, 127, 0), scales=(0.01, 0.01, 0.01 * 0.01 * 130 * 255 * 255 / 120.0),
                                 fill=(127, -128), hint=hint))
    # the transposed reads of a staged operand pinned by hint (8 ds_read_b128 after transposing writes, 16 byte
    # gathers, 32 ds_read_b64_tr_b8), with one and four column tiles: staged rhs, staged lhs, both; K tails; N edges
    for read, rtag in ((8, "b128"), (16, "gather"), (32, "tr8")):
        for nt, ntag in ((2, "nt1"), (4, "nt4")):
            for ax, ay in ((False, False), (True, True), (True, False)):
                cases.append(BmmCase("read_%s_%s_adj_%d%d" % (rtag, ntag, ax, ay), (130, 70) if ax else (70, 130),
                                     (65, 130) if ay else (130, 65), adj_x=ax, adj_y=ay, spread=40,
                                     seed=580 + 2 * ax + ay, hint=read | nt))
            cases.append(BmmCase("read_%s_%s_17x17x15" % (rtag, ntag), (17, 15), (15, 17), spread=40, seed=590,
                                 hint=read | nt))
            cases.append(BmmCase("read_%s_%s_extreme" % (rtag, ntag), (17, 130), (130, 40), zps=(-128, 127, 0),
                                 scales=(0.01, 0.01, 0.01 * 0.01 * 130 * 255 * 255 / 120.0), fill=(127, -128),
                                 hint=read | nt))
        cases.append(BmmCase("read_%s_misaligned" % rtag, (33, 64), (64, 33), spread=40, seed=595, misalign=(0, 1),
                             hint=read))
    # adj_x and adj_y on a 9,000-tile grid: a staged lhs keeps one tile per wave
    cases.append(BmmCase("large_grid_adj_11", (20, 30, 40, 33), (20, 30, 70, 40), adj_x=True, adj_y=True, spread=40,
                         seed=572))
    cases.append(negative_tie_case())
    for ay in (False, True):
        # 9,000 16 x 16 tiles: with adj_y (a K-contiguous rhs) the launcher takes four tiles per wave by itself
        cases.append(BmmCase("large_grid_adjy%d" % ay, (20, 30, 33, 40), (20, 30, 70, 40) if ay else (20, 30, 40, 70), adj_y=ay,
                             spread=40, seed=570 + ay))
    cases += tie_cases() + [left_shift_case(), clamp_case()]
    # 70,000 matrices: blockIdx.z and .y both above one
    cases.append(BmmCase("batch_70000", (7, 10000, 2, 3), (3, 2), zps=(3, -5, 7), scales=(0.05, 0.05, 0.05), spread=40,
                         seed=530))
    return cases


def float_cases():
    cases = []
    for k in (1, 7, 64, 1001):
        for ay in (False, True):
            cases.append(BmmCase("f32_k%d_adjy%d" % (k, ay), (17, k), (19, k) if ay else (k, 19), adj_y=ay,
                                 dtype=np.float32, seed=600 + k))
    cases.append(BmmCase("f32_adj_x", (33, 17), (33, 21), adj_x=True, dtype=np.float32, seed=610))
    m, k, n = 17, 33, 19
    for name, ls, rs in (("bcast_rhs_lead1", (2, 3, m, k), (1, 3, k, n)), ("bcast_rhs_rank3", (2, 3, m, k), (3, k, n)),
                         ("bcast_lhs_mid1", (2, 1, m, k), (2, 3, k, n)), ("rank2_rank2", (m, k), (k, n)),
                         ("rank2_rhs_under_rank4", (2, 3, m, k), (k, n))):
        cases.append(BmmCase("f32_" + name, ls, rs, dtype=np.float32, seed=620 + len(cases)))
    for which in (0, 1):
        c = BmmCase("f32_nan_inf_%s" % "lr"[which], (17, 40), (40, 19), dtype=np.float32, seed=640 + which)
        t = c.lhs if which == 0 else c.rhs
        t[3, 5] = np.nan
        t[9, 11] = np.inf
        t[12, 2] = -np.inf
        cases.append(c)
    return cases


# ---- launcher parameter blocks -----------------------------------------------------
def bmm_params(case, lhs_ptr, rhs_ptr, out_ptr, requant_fast=-1):
    """bh_batch_matmul_params of the case: strides (elements) of the stored, dense operands"""
    from band_amd import _abi
    A, B = case.views()
    p = _abi.BatchMatMulParams()
    p.batch[0], p.batch[1] = A.shape[0], A.shape[1]
    p.m, p.k, p.n = A.shape[2], A.shape[3], B.shape[3]
    for t, bstride in ((case.lhs, p.lhs_bstride), (case.rhs, p.rhs_bstride)):
        lead = (1,) * (4 - t.ndim) + tuple(t.shape[:-2])
        mat = t.shape[-2] * t.shape[-1]
        bstride[0] = lead[1] * mat if lead[0] > 1 else 0  # a dim of 1 broadcasts (or is walked once)
        bstride[1] = mat if lead[1] > 1 else 0
    p.lhs_row_stride, p.lhs_k_stride = (1, case.lhs.shape[-1]) if case.adj_x else (case.lhs.shape[-1], 1)
    p.rhs_k_stride, p.rhs_col_stride = (1, case.rhs.shape[-1]) if case.adj_y else (case.rhs.shape[-1], 1)
    if case.dtype == np.int8:
        p.lhs_zp, p.rhs_zp, p.out_zp, p.mult, p.shift = case.z_l, case.z_r, case.z_o, case.mult, case.shift
    p.requant_fast, p.kernel_hint = requant_fast, case.hint
    p.lhs, p.rhs, p.out = lhs_ptr, rhs_ptr, out_ptr
    return p


def fast_ok(case, lib):
    m, s = ctypes.c_int32(case.mult), ctypes.c_int32(case.shift)
    return lib.bh_conv_requant_fast_ok(ctypes.byref(m), ctypes.byref(s), 1, case.mnk[2], 0)


def launch(case, lib, device, requant_fast=-1):
    """the case through bh_batch_matmul_i8 / _f32 (device) or the host twins;
    the output buffer is 0xff and SLACK bytes longer than the result"""
    from band_amd import _abi
    ml, mr = case.misalign
    raw = [np.concatenate([np.zeros(o, np.uint8), t.view(np.uint8).reshape(-1)]) for o, t in ((ml, case.lhs), (mr, case.rhs))]
    nbytes = int(np.prod(case.out_shape)) * case.lhs.itemsize
    dl, dr, dy = (_buffer(a, device) for a in (raw[0], raw[1], np.full(nbytes + SLACK, 0xff, np.uint8)))
    p = bmm_params(case, dl.value + ml, dr.value + mr, dy.value, requant_fast)
    f32 = case.dtype == np.float32
    if device:
        fn = lib.bh_batch_matmul_f32 if f32 else lib.bh_batch_matmul_i8
        _abi.check(fn(ctypes.byref(p), None), "bh_batch_matmul")
    else:
        assert lib.bhx_cpu_batch_matmul(ctypes.byref(p), int(f32)) == 0, lib.bhx_last_error()
    got = dy.download(np.uint8, (nbytes + SLACK,))
    assert (got[nbytes:] == 0xff).all(), "bytes past the output were written"
    return got[:nbytes].view(case.dtype).reshape(case.out_shape)


def refused_params():
    """[(id, set(p), reason fragment)] on a valid 4 x 5 x 6 int8 block"""
    def setter(**kw):
        def f(p):
            for k, v in kw.items():
                if isinstance(v, tuple):
                    getattr(p, k)[v[0]] = v[1]
                else:
                    setattr(p, k, v)
        return f
    return [("null_lhs", setter(lhs=None), "null"), ("null_out", setter(out=None), "null"),
            ("zero_m", setter(m=0), "non-positive"), ("negative_batch", setter(batch=(0, -1)), "non-positive"),
            ("k_limit", setter(k=32768), "K > 32767"), ("no_unit_stride", setter(lhs_k_stride=2), "unit stride"),
            ("two_unit_strides", setter(rhs_k_stride=1, rhs_col_stride=1), "unit stride"),
            ("index_range", setter(batch=(0, 65535), lhs_bstride=(0, 1 << 31)), "2^31"),
            ("batch_dim", setter(batch=(1, 65536)), "65535")]


def valid_params(lhs_ptr, rhs_ptr, out_ptr):
    case = BmmCase("valid", (4, 6), (6, 5), spread=10, seed=1)
    return bmm_params(case, lhs_ptr, rhs_ptr, out_ptr)


# ---- models ------------------------------------------------------------------------------
def rank2_model():
    """two FULLY_CONNECTED, then BATCH_MATMUL(adj_x) of their rank-2 outputs
    ([1, 24]^T x [1, 24] -> [24, 24], K = 1): runs, but cannot be job-batched"""
    g = QGraph(np.int8, seed=83, name="bmm_rank2")
    x = g.input([1, 24], scale=0.05)
    a = g.fully_connected(x, 24)
    b = g.fully_connected(x, 24)
    g.output(g.batch_matmul(a, b, adj_x=True))
    return g.build()


def const_rhs_model():
    """an activation [1, 2, 9, 16] times a constant rank-2 rhs [16, 12] (uploaded as it is), then RELU"""
    g = QGraph(np.int8, seed=85, name="bmm_const_rhs")
    x = g.input([1, 2, 9, 16], scale=0.05)
    w = g.rng.integers(-127, 128, (16, 12)).astype(np.int8)
    wt = g.mb.tensor("bmm_const", [16, 12], np.int8, scale=[0.01], zero_point=[4], data=w)
    g.meta[wt] = ([16, 12], 0.01, 4)
    g.output(g.relu(g.batch_matmul(x, wt), "RELU6"))
    return g.build()


def one_op_model(lhs_shape, rhs_shape, dtype=np.int8, rhs_dtype=None, out_dtype=None, adj_x=False, adj_y=False,
                 out_shape=None):
    """a BATCH_MATMUL alone with the given tensor types (the refusal models)"""
    from band_amd.tflite_synth import OPT, ModelBuilder, _bmm_shape, bmm_options
    mb = ModelBuilder("bmm_one_op")

    def tensor(name, shape, dt):
        q = {} if np.dtype(dt) == np.float32 else dict(scale=[0.05], zero_point=[0 if np.dtype(dt) != np.uint8 else 128])
        return mb.tensor(name, list(shape), dt, **q)
    a = tensor("a", lhs_shape, dtype)
    b = tensor("b", rhs_shape, rhs_dtype or dtype)
    if out_shape is None:
        try:
            out_shape = _bmm_shape(list(lhs_shape), list(rhs_shape), adj_x, adj_y)[0]
        except AssertionError:
            out_shape = list(lhs_shape[:-1]) + [rhs_shape[-1]]
    y = tensor("y", out_shape, out_dtype or dtype)
    mb.inputs += [a, b]
    mb.op("BATCH_MATMUL", [a, b], [y], OPT["BatchMatMulOptions"], bmm_options(adj_x, adj_y))
    mb.outputs.append(y)
    return mb.build()


MODELS = {
    "attention_17_48_3": lambda: attention_block(np.int8, tokens=17, dim=48, heads=3),
    "attention_64_64_2": lambda: attention_block(np.int8, tokens=64, dim=64, heads=2),
    "attention_f32": lambda: attention_block(np.float32, tokens=17, dim=48, heads=3),
    "vit_tiny_32": lambda: vit_tiny(np.int8, size=32, dim=48, heads=3),
    "const_rhs": const_rhs_model,
}


def eval_bmm(om, o, vals):
    """BATCH_MATMUL operator o on vals: int8 through bmm_eval, float32 as the float64 product"""
    T = om.tensors
    tl, tr, to = T[o.inputs[0]], T[o.inputs[1]], T[o.outputs[0]]
    adj_x = bool(o.options.scalar(0, "b", 0)) if o.options is not None else False
    adj_y = bool(o.options.scalar(1, "b", 0)) if o.options is not None else False
    lhs, rhs = vals[o.inputs[0]], vals[o.inputs[1]]
    if tl.np_dtype == np.float32:
        a = np.swapaxes(lhs, -1, -2) if adj_x else lhs
        b = np.swapaxes(rhs, -1, -2) if adj_y else rhs
        return [np.matmul(a.astype(np.float64), b.astype(np.float64)).astype(np.float32)]
    (s_l, z_l), (s_r, z_r), (s_o, z_o) = orc._q(tl), orc._q(tr), orc._q(to)
    mult, shift = orc.conv_multipliers(s_l, np.array([s_r], np.float32), 1, s_o, True)  # FullyConnectedMultiplier
    return [bmm_eval(lhs, rhs, adj_x, adj_y, z_l, z_r, z_o, int(mult[0]), int(shift[0]))]
