"""Fixtures of the masked form of the fused int8 attention launch (bh_attention_i8
with a bias): the cases, the composed reference, the parameter blocks, the
default sequence of four launches and the models with an ADD on the scores.

Reference: scores = AttnCase.scores() (the oracle's FULLY_CONNECTED per batch
slice), masked = oracle.runner.add of the scores and the bias with
oracle.runner.add_params' constants, p = oracle.runner.softmax of the masked
scores at the ADD output's scale, out = bmm_eval of p and v.  An expected byte
never comes from the product."""
import ctypes

import numpy as np

from oracle import runner as orc
from tests import attention_models as A
from tests import bmm_models as B
from tests.grouped_models import SLACK, _buffer

KERNEL = "attention_bias_i8_kernel"
KEYS = (1, 15, 16, 17, 63, 64, 65, 130)
LAYOUTS = ("padding", "causal", "per_head", "full", "key_broadcast", "scalar")


def bias_shape(layout, batch, rows, keys):
    b0, b1 = batch
    return {"padding": (b0, 1, 1, keys), "causal": (1, 1, rows, keys), "per_head": (1, b1, rows, keys),
            "full": (b0, b1, rows, keys), "key_broadcast": (b0, b1, rows, 1), "scalar": (1, 1, 1, 1)}[layout]


class BiasCase(A.AttnCase):
    """An AttnCase whose scores meet an int8 bias in an ADD before the softmax.  bias: [b0 | 1, b1 | 1, rows | 1,
    keys | 1] int8 at (bias_scale, bias_zp); the ADD's output is at (add_scale, add_zp) within act; operand: which
    ADD input the scores are (0: the first); bias_off: bytes the bias lies off its buffer."""

    def __init__(self, name, batch, rows, keys, head_dim, out_dim, bias="full", bias_scale=0.1, bias_zp=-3,
                 add_scale=0.2, add_zp=5, act=(-128, 127), operand=0, bias_off=0, **kw):
        super().__init__(name, batch, rows, keys, head_dim, out_dim, **kw)
        rng = np.random.default_rng(kw.get("seed", 0) + 7000)
        if isinstance(bias, str):
            bias = rng.integers(-128, 128, bias_shape(bias, self.batch, rows, keys)).astype(np.int8)
        self.bias = np.ascontiguousarray(bias, np.int8)
        assert self.bias.ndim == 4
        self.add_scales = (self.qk_scales[2], bias_scale, add_scale)
        self.z_b, self.z_m, self.act, self.operand, self.bias_off = bias_zp, add_zp, act, operand, bias_off

    @property
    def in_scale(self):
        """the softmax's input scale: the ADD output's"""
        return float(np.float32(self.add_scales[2]))

    def add_consts(self):
        """(m_a, s_a, m_b, s_b, m_o, s_o, left_shift) with a / b the ADD's first / second operand"""
        s_s, s_b, s_m = self.add_scales
        sa, sb = (s_s, s_b) if self.operand == 0 else (s_b, s_s)
        return orc.add_params(sa, sb, s_m)

    def masked(self, scores=None, bias=None, consts=None):
        s = self.scores() if scores is None else scores
        b = self.bias if bias is None else bias
        prm = self.add_consts() if consts is None else consts
        ops = (s, b, self.z_s, self.z_b) if self.operand == 0 else (b, s, self.z_b, self.z_s)
        return orc.add(ops[0], ops[1], a_zp=ops[2], b_zp=ops[3], out_zp=self.z_m, params=prm, amin=self.act[0],
                       amax=self.act[1])

    def ctx(self, masked):
        return B.bmm_eval(self.probs(masked), self.v, False, False, self.z_p, self.z_v, self.z_o, self.pv_mult,
                          self.pv_shift)

    def ref(self):
        return self.ctx(self.masked())


def saturation_case():
    """keys 70, rows 33, head_dim 65: scores about 12 LSBs wide at scale 0.1, the bias uniform over -128 .. 127 at
    scale 0.08 (not the scores' 0.1: equal input scales give equal input multipliers, and exchanging them would
    be no mistake), the ADD output at 0.05: about a fifth of the masked scores at each bound"""
    return BiasCase("saturates", (2, 2), 33, 70, 65, 16, bias="full", bias_scale=0.08, bias_zp=0, add_scale=0.05,
                    add_zp=0, seed=610)


def padding_case():
    """a padding mask [b0, 1, 1, keys] at scale 10000 / 255, zero point 127 (127: a token, -128: padding) on keys
    33: item 0 has every key masked, item 1 the keys from 20 on; the ADD output has the scores' quantisation"""
    c = BiasCase("padding_rows", (2, 3), 17, 33, 36, 36, bias=np.full((2, 1, 1, 33), 127, np.int8),
                 bias_scale=10000.0 / 255, bias_zp=127, add_scale=0.1, add_zp=7, seed=620)
    c.bias[0] = -128
    c.bias[1, 0, 0, PAD_FROM:] = -128
    return c


PAD_FROM = 20


def identity_case():
    """sum_order()'s rows under a bias at its zero point and ADD scales equal to the scores': the ADD is the
    identity, so the in-order row sum is still what decides the bytes.  Returns (case, reversed rows, pairwise rows)"""
    base, rev, pair = A.sum_order()
    c = BiasCase("sum_order_identity", base.batch, base.rows, base.keys, base.head_dim, base.out_dim,
                 bias=np.full((1, 1, 1, base.keys), -9, np.int8), bias_scale=base.qk_scales[2], bias_zp=-9,
                 add_scale=base.qk_scales[2], add_zp=base.z_s, qk_scales=base.qk_scales, seed=900)
    c.q, c.k, c.v = base.q, base.k, base.v
    return c, rev, pair


def launcher_cases():
    cases = []
    for i, layout in enumerate(LAYOUTS):
        cases.append(BiasCase("layout_" + layout, (2, 3), 17, 33, 36, 36, bias=layout, seed=500 + i))
    for i, keys in enumerate(KEYS):
        cases.append(BiasCase("keys_%d" % keys, (1, 2), 17, keys, 36, 36, bias="full", seed=520 + i))
    cases.append(BiasCase("keys_1024_rows_65", (1, 1), 65, 1024, 64, 32, bias="full", seed=540))
    for off in (1, 4):
        cases.append(BiasCase("bias_off_%d" % off, (1, 2), 17, 64, 64, 32, bias="full", bias_off=off, seed=550 + off))
    cases.append(BiasCase("bias_bytes_hint", (1, 2), 17, 64, 64, 32, bias="full", hint=1, seed=556))
    cases.append(BiasCase("padding_dwords", (2, 3), 17, 64, 64, 32, bias="padding", seed=557))
    cases.append(BiasCase("heads_layout", (2, 3), 17, 33, 36, 36, bias="per_head", layout="heads", seed=560))
    cases.append(BiasCase("heads_65x130", (1, 3), 65, 130, 64, 64, bias="causal", layout="heads", seed=561))
    cases.append(BiasCase("scores_second", (2, 3), 17, 33, 36, 36, bias="full", operand=1, bias_scale=0.07, seed=570))
    cases.append(BiasCase("narrow_window", (2, 3), 17, 33, 36, 36, bias="full", act=(-20, 41), seed=580))
    cases.append(BiasCase("bcast_kv", (2, 3), 17, 33, 16, 16, bias="padding", kv_batch=(1, 1), seed=590))
    cases += [saturation_case(), padding_case(), identity_case()[0]]
    return cases


# ---- launcher parameter blocks -----------------------------------------------------------
def set_bias(p, case, ptr):
    """the masked form's fields of an AttentionParams: dense strides of the bias, 0 for an extent of 1"""
    shape = case.bias.shape
    dense = [int(np.prod(shape[d + 1:])) for d in range(4)]
    st = [0 if shape[d] == 1 else dense[d] for d in range(4)]
    p.bias = ptr
    p.bias_bstride[0], p.bias_bstride[1], p.bias_row_stride, p.bias_key_stride = st
    a = p.add
    a.a_mult, a.a_shift, a.b_mult, a.b_shift, a.o_mult, a.o_shift, a.left_shift = [int(v) for v in case.add_consts()]
    zs = (case.z_s, case.z_b) if case.operand == 0 else (case.z_b, case.z_s)
    a.a_off, a.b_off, a.o_off = -zs[0], -zs[1], case.z_m
    a.act_min, a.act_max = case.act
    p.add_scores_operand = case.operand
    return p


def prepare(case, device, requant_fast=-1):
    """attention_models.prepare plus the bias in a buffer of its own, bias_off bytes in"""
    p, bufs, read = A.prepare(case, device, requant_fast)
    raw = np.concatenate([np.zeros(case.bias_off, np.uint8), case.bias.view(np.uint8).reshape(-1)])
    bb = _buffer(raw, device)
    set_bias(p, case, bb.value + case.bias_off)
    return p, bufs + [bb], read


def launch(case, lib, requant_fast=-1):
    """the case through bh_attention_i8 (kernel name asserted first)"""
    from band_amd import _abi
    p, bufs, read = prepare(case, True, requant_fast)
    assert lib.bh_attention_i8_kernel(ctypes.byref(p)) == KERNEL.encode(), lib.bh_last_error()
    _abi.check(lib.bh_attention_i8(ctypes.byref(p), None), "bh_attention_i8")
    return read()


def _lead_strides(shape):
    mat = shape[-2] * shape[-1]
    return (shape[1] * mat if shape[0] > 1 else 0, mat if shape[1] > 1 else 0)


def launch_default_sequence(case, lib, requant_fast=-1):
    """the case's logical tensors through bh_batch_matmul_i8 -> bh_eltwise_i8 (ADD) -> bh_softmax_i8 ->
    bh_batch_matmul_i8, every tensor dense: (masked scores, context)"""
    from band_amd import _abi
    from band_amd.device import DeviceBuffer
    b0, b1 = case.batch
    R, K, D, N = case.rows, case.keys, case.head_dim, case.out_dim
    dq, dk, dv, db = (DeviceBuffer.from_array(np.ascontiguousarray(t)) for t in (case.q, case.k, case.v, case.bias))
    n_sc = b0 * b1 * R * K
    d_sc, d_m, d_p = DeviceBuffer(n_sc), DeviceBuffer(n_sc), DeviceBuffer(n_sc)
    d_o = DeviceBuffer(b0 * b1 * R * N)
    tab = DeviceBuffer.from_array(orc.softmax_table(case.in_scale, 1.0))

    def bmm(lhs, lshape, rhs, rshape, out, m, k, n, adj_y, zps, mult, shift):
        p = _abi.BatchMatMulParams()
        p.batch[0], p.batch[1], p.m, p.k, p.n = b0, b1, m, k, n
        p.lhs_bstride[0], p.lhs_bstride[1] = _lead_strides(lshape)
        p.rhs_bstride[0], p.rhs_bstride[1] = _lead_strides(rshape)
        p.lhs_row_stride, p.lhs_k_stride = k, 1
        p.rhs_k_stride, p.rhs_col_stride = (1, k) if adj_y else (n, 1)
        p.lhs_zp, p.rhs_zp, p.out_zp, p.mult, p.shift = zps + (mult, shift)
        p.requant_fast, p.kernel_hint = requant_fast, 0
        p.lhs, p.rhs, p.out = lhs.value, rhs.value, out.value
        _abi.check(lib.bh_batch_matmul_i8(ctypes.byref(p), None), "bh_batch_matmul_i8")
    bmm(dq, case.q.shape, dk, case.k.shape, d_sc, R, D, K, True, (case.z_q, case.z_k, case.z_s), case.qk_mult,
        case.qk_shift)
    e = _abi.EltwiseParams()
    e.kind, e.in_signed = 0, 1
    sa, sb = ((b0, b1, R, K), case.bias.shape) if case.operand == 0 else (case.bias.shape, (b0, b1, R, K))
    for i in range(4):
        e.shape_a[i], e.shape_b[i], e.shape_o[i] = sa[i], sb[i], (b0, b1, R, K)[i]
    att = _abi.AttentionParams()
    set_bias(att, case, None)
    for f in ("a_off", "b_off", "o_off", "left_shift", "a_mult", "a_shift", "b_mult", "b_shift", "o_mult", "o_shift",
              "act_min", "act_max"):
        setattr(e, f, getattr(att.add, f))
    e.a, e.b = (d_sc.value, db.value) if case.operand == 0 else (db.value, d_sc.value)
    e.out = d_m.value
    _abi.check(lib.bh_eltwise_i8(ctypes.byref(e), None), "bh_eltwise_i8")
    s = _abi.SoftmaxParams()
    s.rows, s.depth, s.is_signed, s.table = b0 * b1 * R, K, 1, tab.value
    s.out_scale, s.out_zp, s.input, s.output = 1.0 / 256, case.z_p, d_m.value, d_p.value
    _abi.check(lib.bh_softmax_i8(ctypes.byref(s), None), "bh_softmax_i8")
    bmm(d_p, (b0, b1, R, K), dv, case.v.shape, d_o, R, K, N, False, (case.z_p, case.z_v, case.z_o), case.pv_mult,
        case.pv_shift)
    return d_m.download(np.int8, (b0, b1, R, K)), d_o.download(np.int8, (b0, b1, R, N))


def refused_params():
    """[(id, change(p), reason fragment)] on valid_case()'s block: the masked form's own refusals"""
    def setter(**kw):
        def f(p):
            for k, v in kw.items():
                if isinstance(v, tuple):
                    getattr(p, k)[v[0]] = v[1]
                else:
                    setattr(p, k, v)
        return f

    def add(**kw):
        def f(p):
            for k, v in kw.items():
                setattr(p.add, k, v)
        return f
    return [("negative_row_stride", setter(bias_row_stride=-7), "negative bias stride"),
            ("negative_batch_stride", setter(bias_bstride=(0, -1)), "negative bias stride"),
            ("negative_key_stride", setter(bias_key_stride=-1), "negative bias stride"),
            ("key_stride_2", setter(bias_key_stride=2), "key stride other than 0 or 1"),
            ("bias_span", setter(batch=(0, 65535), bias_bstride=(0, 1 << 31)), "bias of 2^31"),
            ("a_shift_positive", add(a_shift=1), "ADD input shift above 0"),
            ("b_shift_positive", add(b_shift=2), "ADD input shift above 0"),
            ("o_shift_positive", add(o_shift=1), "ADD shift outside"),
            ("a_shift_deep", add(a_shift=-32), "ADD shift outside"),
            ("left_shift_negative", add(left_shift=-1), "left_shift outside 0 .. 31"),
            ("left_shift_32", add(left_shift=32), "left_shift outside 0 .. 31"),
            ("empty_window", add(act_min=5, act_max=4), "act_min > act_max"),
            ("operand_2", setter(add_scores_operand=2), "add_scores_operand")]


def valid_case():
    return BiasCase("valid", (1, 2), 5, 7, 16, 16, bias="full", seed=1)


# ---- models --------------------------------------------------------------------------------
def padded_block(tokens=17, dim=48, heads=3, batch=2, seed=12):
    """attention_block with a second input: an int8 padding mask [batch, 1, 1, tokens] at scale 10000 / 255, zero
    point 127 (127: a token, -128: padding), ADDed to every head's scores: a runtime bias, read by one ADD here"""
    from band_amd.tflite_synth import MASKED, QGraph, _attention
    g = QGraph(np.int8, seed, "padded_attention_block")
    x = g.input([batch, tokens, dim], scale=0.05)
    m = g.input([batch, 1, 1, tokens], scale=-MASKED / 255.0, zp=127)
    g.output(_attention(g, x, heads, bias=m))
    return g.build()


def padded_encoder(tokens=17, dim=48, heads=3, hidden=96, batch=1, seed=13):
    """encoder_block with padded_block's mask input on its attention"""
    from band_amd.tflite_synth import MASKED, QGraph, _encoder
    g = QGraph(np.int8, seed, "padded_encoder_block")
    x = g.input([batch, tokens, dim], scale=0.05)
    m = g.input([batch, 1, 1, tokens], scale=-MASKED / 255.0, zp=127)
    g.output(_encoder(g, x, heads, hidden, bias=m))
    return g.build()


def _block(kind, tokens=17, dim=48, heads=3):
    def build():
        from band_amd.tflite_synth import attention_block
        return attention_block(np.int8, tokens=tokens, dim=dim, heads=heads, attention_bias=kind)
    return build


MODELS = {"causal_17_48_3": _block("causal"), "relative_17_48_3": _block("relative"),
          "relative_65_64_2": _block("relative", 65, 64, 2), "padded_17_48_3": padded_block,
          "padded_one_17_48_3": lambda: padded_block(batch=1),  # (job batching takes a unit batch dimension)
          "padded_encoder_17_48_3_96": padded_encoder}
PADDED = (5, 0)  # masked tokens at the end of the two batch items of padded_block


def unfusable_model(kind):
    """BATCH_MATMUL(x, x, adj_y) -> an 8-bit eltwise op on the scores -> SOFTMAX -> BATCH_MATMUL on one input
    [1, tokens, 8]: four consecutive launches of the masked pattern's kinds that FuseAttention must leave alone.
    kind: "sub" (SUB of a constant bias: not an ADD), "scores_twice" (ADD(scores, scores): not exactly one operand
    is the scores), "over_limit" (ADD of a constant bias at keys 1,025: the launcher's check refuses)"""
    from band_amd.tflite_synth import QGraph
    tokens = 1025 if kind == "over_limit" else 17
    g = QGraph(np.int8, seed=93, name="unfusable_" + kind)
    x = g.input([1, tokens, 8], scale=0.05)
    sc = g.batch_matmul(x, x, adj_y=True)
    _, s, z = g.meta[sc]
    lo, hi = -128, 127
    q = np.random.default_rng(94).integers(lo, hi + 1, (1, 1, tokens))
    b = g.const_at((q - z) * s, s, z, "bias")
    if kind == "sub":
        m = g.sub(sc, b, s, z)
    elif kind == "scores_twice":
        m = g.add_q(sc, sc, s, z)
    else:
        m = g.add_q(sc, b, s, z)
    g.output(g.batch_matmul(g.softmax(m, beta=1.0), x, out_scale=0.05))
    return g.build()


UNFUSABLE = ("sub", "scores_twice", "over_limit")


def model_inputs(buf, seed=0):
    """{input tensor: array}: activations within +-60 LSB of the zero point; a padding mask (an input of shape
    [batch, 1, 1, tokens]) with PADDED[b % 2] trailing tokens masked in item b"""
    from oracle.tflite_fb import Model as OModel
    om = OModel(buf)
    rng = np.random.default_rng(seed)
    out = {}
    for i in om.inputs:
        t = om.tensors[i]
        shape = tuple(t.shape)
        if len(shape) == 4 and shape[1:3] == (1, 1):
            m = np.full(shape, 127, np.int8)
            for b in range(shape[0]):
                n = PADDED[(b + seed) % 2]
                if n:
                    m[b, 0, 0, -n:] = -128
            out[i] = m
        else:
            z = int(t.zero_point[0])
            lo, hi = (0, 255) if t.np_dtype == np.uint8 else (-128, 127)
            out[i] = np.clip(z + np.round(rng.normal(0, 30, shape)), lo, hi).astype(t.np_dtype)
    return out


def masked_attention_tensors(buf):
    """per masked attention of the model: (scores, masked scores, probabilities, context, bias) tensor indices"""
    from oracle.tflite_fb import Model as OModel
    ops = OModel(buf).operators
    out = []
    for i in range(len(ops) - 3):
        a, e, s, b = ops[i:i + 4]
        if (a.builtin, e.builtin, s.builtin, b.builtin) == (B.BATCH_MATMUL, 0, 25, B.BATCH_MATMUL):
            sc = a.outputs[0]
            bias = e.inputs[1] if e.inputs[0] == sc else e.inputs[0]
            out.append((sc, e.outputs[0], s.outputs[0], b.outputs[0], bias))
    return out
