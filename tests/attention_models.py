"""Fixtures of the fused int8 attention launch (bh_attention_i8): the cases, the
composed reference, the parameter blocks, the directed sum-order case and the
models.

Reference: scores = tests.bmm_models.bmm_eval (the oracle's FULLY_CONNECTED per
batch slice) of q and k with adj_y, p = oracle.runner.softmax of the scores,
out = bmm_eval of p and v.  An expected byte never comes from the product.

np_softmax is a numpy restatement of the 8-bit softmax whose row sum can be
taken in order (the reference's), reversed or pairwise; the CPU test holds the
in-order form against the oracle and shows on the sum-order case that the other
two store different bytes."""
import ctypes

import numpy as np

from band_amd.tflite_synth import QGraph, attention_block, encoder_block, vit_tiny
from oracle import runner as orc
from tests import bmm_models as B
from tests.fixed_point import round_half_away
from tests.grouped_models import SLACK, _buffer

KERNEL = "attention_i8_kernel"
ROWS = (1, 15, 16, 17, 63, 64, 65, 130)
KEYS = (1, 15, 16, 17, 63, 64, 65, 130, 196, 1024)
HEAD_DIMS = (1, 15, 16, 36, 64, 65, 128)
OUT_DIMS = (1, 3, 16, 36, 64, 128)
SIGMA40 = 23.4  # standard deviation of integers uniform in -40 .. 40


def _mult(s_l, s_r, s_o):
    """FullyConnectedMultiplier: the float32 product of the input scales over the output scale, in double"""
    return orc.quantize_multiplier(float(np.float32(s_l) * np.float32(s_r)) / float(np.float32(s_o)))


def score_scales(head_dim, lsb, spread=40, s_out=0.1):
    """(s_q, s_k, s_scores) that put Q K^T of +-spread operands about `lsb` score LSBs wide"""
    sigma = SIGMA40 * spread / 40.0
    m = lsb / (np.sqrt(head_dim) * sigma * sigma)
    s = float(np.sqrt(s_out * m))
    return (s, s, s_out)


class AttnCase:
    """q [b0, b1, rows, D], k [.., keys, D], v [.., keys, out_dim] as the kernel sees them (k and v may have
    leading dims of 1: a broadcast).  layout: "dense", or "heads" (q, k, v and out stored [b0, T, b1, D], the
    operands of absorbed head TRANSPOSEs).  misalign: bytes q, k, v and out lie off their buffers."""

    def __init__(self, name, batch, rows, keys, head_dim, out_dim, zps=(3, -5, 7), qk_scales=None, lsb=12.0,
                 spread=40, v_zp=-5, out_zp=4, pv_scales=(1.0 / 256, 0.03, 0.028), layout="dense", kv_batch=None,
                 misalign=(0, 0, 0, 0), hint=0, fill=None, seed=0):
        self.name, self.layout, self.misalign, self.hint = name, layout, misalign, hint
        rng = np.random.default_rng(seed)
        self.z_q, self.z_k, self.z_s = zps
        kvb = tuple(batch) if kv_batch is None else tuple(kv_batch)

        def draw(shape, zp, which):
            if fill is not None and fill[which] is not None:
                return np.full(shape, fill[which], np.int8)
            return np.clip(zp + rng.integers(-spread, spread + 1, shape), -128, 127).astype(np.int8)
        self.q = draw(tuple(batch) + (rows, head_dim), self.z_q, 0)
        self.k = draw(kvb + (keys, head_dim), self.z_k, 1)
        self.v = np.clip(v_zp + rng.integers(-100, 101, kvb + (keys, out_dim)), -128, 127).astype(np.int8)
        self.qk_scales = score_scales(head_dim, lsb, spread) if qk_scales is None else qk_scales
        self.qk_mult, self.qk_shift = _mult(*self.qk_scales)
        self.z_p, self.z_v, self.z_o = -128, v_zp, out_zp
        self.pv_scales = pv_scales
        self.pv_mult, self.pv_shift = _mult(*pv_scales)
        self.batch, self.rows, self.keys, self.head_dim, self.out_dim = tuple(batch), rows, keys, head_dim, out_dim

    @property
    def in_scale(self):
        return float(np.float32(self.qk_scales[2]))

    def scores(self):
        return B.bmm_eval(self.q, self.k, False, True, self.z_q, self.z_k, self.z_s, self.qk_mult, self.qk_shift)

    def probs(self, scores=None):
        s = self.scores() if scores is None else scores
        return orc.softmax(s, in_scale=self.in_scale, beta=1.0, out_scale=1.0 / 256, out_zp=self.z_p)

    def ref(self):
        return B.bmm_eval(self.probs(), self.v, False, False, self.z_p, self.z_v, self.z_o, self.pv_mult, self.pv_shift)


# ---- a numpy restatement of the 8-bit softmax with the row sum's order as a parameter ----
def np_softmax(x, in_scale, order="forward", out_scale=1.0 / 256, out_zp=-128):
    """int8 x [rows, depth]: table gather, float32 row sum in `order` (forward: j = 0 .. depth - 1 from 0.0f, the
    reference's; reversed; pairwise: adjacent pairs, level by level), 1 / (sum * out_scale), round, clamp"""
    x = np.asarray(x, np.int8)
    table = orc.softmax_table(in_scale, 1.0)
    mx = x.max(axis=-1, keepdims=True).astype(np.int32)
    e = table[255 - mx + x.astype(np.int32)]
    if order == "pairwise":
        level = e
        while level.shape[-1] > 1:
            if level.shape[-1] % 2:
                level = np.concatenate([level, np.zeros(level.shape[:-1] + (1,), np.float32)], axis=-1)
            level = (level[..., 0::2] + level[..., 1::2]).astype(np.float32)
        s = level[..., 0]
    else:
        cols = range(e.shape[-1]) if order == "forward" else range(e.shape[-1] - 1, -1, -1)
        s = np.zeros(e.shape[:-1], np.float32)
        for j in cols:
            s = (s + e[..., j]).astype(np.float32)
    inv = (np.float32(1.0) / (s * np.float32(out_scale)).astype(np.float32)).astype(np.float32)
    pr = (e * inv[..., None]).astype(np.float32)
    return np.clip(round_half_away(pr).astype(np.int32) + out_zp, -128, 127).astype(np.int8)


SUM_ORDER_FLOOR = 32


def sum_order_case(floor=SUM_ORDER_FLOOR, candidates=3000):
    """keys 196, head_dim 64, scores at scale 0.1.  Random rows almost never tell the orders of the row sum apart
    (about 1 in 50,000 here), so the candidates are directed: K is one-hot (key j has a 1 above its zero point in
    dimension g(j): 100 keys in group 0, 96 in groups 1 .. 63) and the multiplier is 1, so score[i][j] is
    q[i][g(j)] shifted by the zero points and a q row sets the 64 group scores freely.  Group 0 holds the row
    maximum, so its probability is 256 / sum; the other groups' scores are chosen (a random prefix, then greedily)
    so that the exact sum lands on 512 / 3 or 512 / 5, a rounding tie of that probability: which side the float32
    sum falls on depends on its order.  A seeded set of such rows is evaluated and the rows whose probabilities
    change when the sum is reversed, and those where they change when it is pairwise, are kept, `floor` of each.
    Returns (case, reversed_rows, pairwise_rows): row indices into the case's q."""
    s01 = float(np.sqrt(0.1))
    proto = AttnCase("sum_order", (1, 1), 1, 196, 64, 36, qk_scales=(s01, s01, 0.1), seed=900)
    rng = np.random.default_rng(901)
    sizes = np.array([100] + [2] * 33 + [1] * 30)
    group = rng.permutation(np.repeat(np.arange(64), sizes))
    proto.k = np.full((1, 1, 196, 64), proto.z_k, np.int8)
    proto.k[0, 0, np.arange(196), group] += 1
    table = orc.softmax_table(proto.in_scale, 1.0).astype(np.float64)
    asc = table[255 - 240:255]  # e(delta) for delta = 240 .. 1, ascending
    top, C = 120, candidates
    target = 512.0 / (2 * rng.integers(1, 3, C) + 1) - 100.0
    deltas = np.zeros((C, 64), np.int64)
    order = np.argsort(rng.random((C, 63)), axis=1) + 1
    prefix = rng.integers(0, 20, C)
    left = target.copy()
    for step in range(63):
        g = order[:, step]
        n = np.searchsorted(asc, left / sizes[g], side="right")  # table values that fit
        d = np.where(n > 0, 241 - n, 240)
        d = np.where(step < prefix, np.maximum(d, rng.integers(1, 50, C)), d)
        deltas[np.arange(C), g] = d
        left -= sizes[g] * table[255 - d]
    scores = (top - deltas)[:, group].astype(np.int8)
    base = np_softmax(scores, proto.in_scale)
    keep = []
    for order_ in ("reversed", "pairwise"):
        hit = np.nonzero((np_softmax(scores, proto.in_scale, order_) != base).any(axis=-1))[0]
        keep.append(hit[:floor])
    rows = np.concatenate(keep)
    proto.q = (proto.z_q + top - deltas[rows] - proto.z_s).astype(np.int8).reshape(1, 1, len(rows), 64)
    proto.rows = len(rows)
    return proto, np.arange(len(keep[0])), len(keep[0]) + np.arange(len(keep[1]))


_SUM_ORDER = []


def sum_order():
    """sum_order_case(), searched once per process"""
    if not _SUM_ORDER:
        _SUM_ORDER.append(sum_order_case())
    return _SUM_ORDER[0]


# ---- the launcher cases ----------------------------------------------------------------
def covering_extents():
    """10 (rows, keys, head_dim, out_dim): every value of the four lists at least once"""
    return [(ROWS[i % 8], KEYS[i], HEAD_DIMS[i % 7], OUT_DIMS[i % 6]) for i in range(10)] + [(130, 130, 128, 128)]


def clamp_case():
    """head_dim 65 at 0.02 x 0.03 / 0.05 with operands within +-56 of their zero points (bmm_models.clamp_case's
    distribution): scores saturate at both bounds"""
    return AttnCase("clamps", (1, 2), 33, 70, 65, 16, zps=(5, -7, 2), qk_scales=(0.02, 0.03, 0.05), spread=56, seed=420)


def flat_case():
    """q at its zero point: every accumulator is 0, every score the scores' zero point, every row flat"""
    return AttnCase("flat_rows", (1, 1), 17, 70, 16, 16, fill=(3, None), seed=430)


def peak_case(first):
    """the row maximum at the first / the last key: that key's k row is aligned with q, the others against it"""
    c = AttnCase("max_at_%s_key" % ("first" if first else "last"), (1, 1), 17, 70, 16, 16, lsb=30.0, seed=440 + first)
    c.q[...] = c.z_q + 30
    c.k[...] = c.z_k - 30
    c.k[0, 0, 0 if first else -1] = c.z_k + 30
    return c


def launcher_cases():
    cases = []
    for i, (r, k, h, o) in enumerate(covering_extents()):
        cases.append(AttnCase("ext_%dx%dx%dx%d" % (r, k, h, o), (1, 1), r, k, h, o, seed=100 + i))
    for batch in ((2, 3), (1, 5)):
        for layout in ("dense", "heads"):
            cases.append(AttnCase("batch_%dx%d_%s" % (batch + (layout,)), batch, 17, 33, 36, 36, layout=layout,
                                  seed=200 + batch[1]))
    cases.append(AttnCase("heads_65x130x64x64", (1, 3), 65, 130, 64, 64, layout="heads", seed=210))
    cases.append(AttnCase("heads_odd_dim", (2, 3), 17, 19, 15, 3, layout="heads", seed=211))  # byte units, byte stores
    cases.append(AttnCase("bcast_kv", (2, 3), 17, 33, 16, 16, kv_batch=(1, 1), seed=220))
    cases.append(AttnCase("bcast_kv_lead", (2, 3), 17, 33, 16, 16, kv_batch=(1, 3), seed=221))
    for which in range(4):
        for off in (1, 4):
            mis = tuple(off if w == which else 0 for w in range(4))
            cases.append(AttnCase("misaligned_%s%d" % ("qkvo"[which], off), (1, 2), 17, 70, 64, 32, misalign=mis,
                                  seed=300 + 2 * which + off))
    cases.append(AttnCase("bytes_hint", (1, 1), 17, 70, 80, 16, hint=1, seed=310))
    cases.append(AttnCase("vec16_tail", (1, 1), 17, 70, 80, 16, seed=310))
    ext = 0.01 * 0.01 * 128 * 255 * 255 / 120.0
    for zq, zk, fq, fk in ((-128, 127, 127, -128), (127, -128, -128, 127), (0, 0, 127, -128), (-128, 127, -128, 127)):
        cases.append(AttnCase("extreme_z%d_%d_q%d_k%d" % (zq, zk, fq, fk), (1, 1), 17, 130, 128, 16, zps=(zq, zk, 0),
                              qk_scales=(0.01, 0.01, ext), fill=(fq, fk), seed=320))
    # all-extreme probabilities against an all-extreme V at both zero points' ends: one key, so p = 127 everywhere
    for zv, fv in ((127, -128), (-128, 127)):
        c = AttnCase("extreme_v_z%d_v%d" % (zv, fv), (1, 1), 17, 1, 16, 16, v_zp=zv, pv_scales=(1.0 / 256, 0.01, 0.02),
                     seed=330)
        c.v[...] = fv
        cases.append(c)
    cases.append(AttnCase("v_zp_0", (1, 2), 17, 70, 36, 36, v_zp=0, seed=340))
    cases.append(AttnCase("qk_left_shift", (1, 1), 17, 33, 33, 16, zps=(2, -1, -3), qk_scales=(0.5, 0.5, 0.1), spread=1,
                          seed=350))
    cases.append(AttnCase("pv_left_shift", (1, 1), 17, 33, 16, 16, pv_scales=(1.0 / 256, 0.5, 0.001), out_zp=-100,
                          seed=351))
    cases.append(AttnCase("table_underflows", (1, 1), 17, 130, 64, 16, qk_scales=score_scales(64, 40.0, s_out=2.0),
                          seed=360))
    cases += [clamp_case(), flat_case(), peak_case(True), peak_case(False)]
    return cases


# ---- launcher parameter blocks -----------------------------------------------------------
def _store(case, logical, off):
    """(storage bytes, the logical view's strides in elements) of a [b0, b1, R, C] operand in the case's layout"""
    if case.layout == "heads":
        stored = np.ascontiguousarray(logical.transpose(0, 2, 1, 3))  # [b0, R, b1, C]
        view = stored.transpose(0, 2, 1, 3)
    else:
        stored = view = np.ascontiguousarray(logical)
    strides = [0 if logical.shape[d] == 1 and d < 2 else view.strides[d] for d in range(4)]
    raw = np.concatenate([np.zeros(off, np.uint8), stored.view(np.uint8).reshape(-1)])
    return raw, strides


def attn_params(case, ptrs, table_ptr, strides, requant_fast=-1):
    from band_amd import _abi
    p = _abi.AttentionParams()
    p.batch[0], p.batch[1] = case.batch
    p.rows, p.keys, p.head_dim, p.out_dim = case.rows, case.keys, case.head_dim, case.out_dim
    for name, st in zip("qkv", strides[:3]):
        bs = getattr(p, name + "_bstride")
        bs[0], bs[1] = st[0], st[1]
        setattr(p, name + "_row_stride", st[2])
        setattr(p, name + "_inner_stride", st[3])
    so = strides[3]
    p.out_bstride[0], p.out_bstride[1], p.out_row_stride, p.out_inner_stride = so
    p.qk = _abi.AttentionQuant(case.z_q, case.z_k, case.z_s, case.qk_mult, case.qk_shift, requant_fast)
    p.pv = _abi.AttentionQuant(case.z_p, case.z_v, case.z_o, case.pv_mult, case.pv_shift, requant_fast)
    p.table, p.sm_out_scale, p.sm_out_zp, p.kernel_hint = table_ptr, 1.0 / 256, case.z_p, case.hint
    p.q, p.k, p.v, p.out = ptrs
    return p


def prepare(case, device, requant_fast=-1):
    """(params, buffers, read): the case's operands in 0-filled buffers, the output in a 0xff buffer SLACK bytes
    longer than the result; read() returns the output as [b0, b1, rows, out_dim] after checking the tail"""
    offs = case.misalign
    out_shape = case.batch + (case.rows, case.out_dim)
    stored = [_store(case, t, o) for t, o in ((case.q, offs[0]), (case.k, offs[1]), (case.v, offs[2]))]
    oraw, ostr = _store(case, np.zeros(out_shape, np.int8), offs[3])
    nbytes = oraw.size
    bufs = [_buffer(s[0], device) for s in stored] + [_buffer(np.full(nbytes + SLACK, 0xff, np.uint8), device),
                                                      _buffer(orc.softmax_table(case.in_scale, 1.0), device)]
    ptrs = [b.value + o for b, o in zip(bufs[:4], offs)]
    p = attn_params(case, ptrs, bufs[4].value, [s[1] for s in stored] + [ostr], requant_fast)

    def read():
        got = bufs[3].download(np.uint8, (nbytes + SLACK,))
        assert (got[nbytes:] == 0xff).all(), "bytes past the output were written"
        assert (got[:offs[3]] == 0xff).all(), "bytes before the output were written"
        body = got[offs[3]:nbytes].view(np.int8)
        if case.layout == "heads":
            b0, b1 = case.batch
            return body.reshape(b0, case.rows, b1, case.out_dim).transpose(0, 2, 1, 3)
        return body.reshape(out_shape)
    return p, bufs, read


def launch(case, lib, requant_fast=-1):
    """the case through bh_attention_i8 (kernel name asserted first)"""
    from band_amd import _abi
    p, bufs, read = prepare(case, True, requant_fast)
    assert lib.bh_attention_i8_kernel(ctypes.byref(p)) == KERNEL.encode(), lib.bh_last_error()
    _abi.check(lib.bh_attention_i8(ctypes.byref(p), None), "bh_attention_i8")
    return read()


def refused_params():
    """[(id, change(p), reason fragment)] on a valid block"""
    def setter(**kw):
        def f(p):
            for k, v in kw.items():
                if isinstance(v, tuple):
                    getattr(p, k)[v[0]] = v[1]
                else:
                    setattr(p, k, v)
        return f
    return [("null_q", setter(q=None), "null pointer"), ("null_out", setter(out=None), "null pointer"),
            ("null_table", setter(table=None), "null pointer"), ("zero_rows", setter(rows=0), "non-positive"),
            ("negative_keys", setter(keys=-1), "non-positive"), ("zero_batch", setter(batch=(1, 0)), "non-positive"),
            ("keys_limit", setter(keys=1025), "keys above 1024"), ("head_dim_limit", setter(head_dim=129), "head_dim above 128"),
            ("out_dim_limit", setter(out_dim=129), "out_dim above 128"), ("batch_dim", setter(batch=(0, 65536)), "65535"),
            ("negative_stride", setter(k_row_stride=-16), "negative stride"),
            ("negative_batch_stride", setter(out_bstride=(1, -4)), "negative stride"),
            ("inner_stride", setter(v_inner_stride=2), "non-unit inner stride"),
            ("index_range", setter(batch=(0, 65535), q_bstride=(0, 1 << 31)), "2^31"),
            ("shift_range", lambda p: setattr(p.pv, "shift", 31), "multiplier / shift")]


def valid_case():
    return AttnCase("valid", (1, 2), 5, 7, 16, 16, seed=1)


# ---- models --------------------------------------------------------------------------------
def shared_operand_model(tokens):
    """BATCH_MATMUL(x, x, adj_y) -> SOFTMAX -> BATCH_MATMUL(p, x) on one input [1, tokens, 8]: one op each, q, k
    and v the same tensor; keys = tokens"""
    g = QGraph(np.int8, seed=91, name="attention_shared_%d" % tokens)
    x = g.input([1, tokens, 8], scale=0.05)
    p = g.softmax(g.batch_matmul(x, x, adj_y=True), beta=1.0)
    g.output(g.batch_matmul(p, x, out_scale=0.05))
    return g.build()


MODELS = {
    "attention_17_48_3": lambda: attention_block(np.int8, tokens=17, dim=48, heads=3),
    "attention_64_64_2": lambda: attention_block(np.int8, tokens=64, dim=64, heads=2),
    "encoder_17_48_3_96": lambda: encoder_block(np.int8, tokens=17, dim=48, heads=3, hidden=96),
    "vit_tiny_32": lambda: vit_tiny(np.int8, size=32, dim=48, heads=3),
    "shared_operand_64": lambda: shared_operand_model(64),
}
ATTENTIONS = {"attention_17_48_3": 1, "attention_64_64_2": 1, "encoder_17_48_3_96": 1, "vit_tiny_32": 2,
              "shared_operand_64": 1}


def attention_tensors(buf):
    """per attention of the model: (scores, probabilities, context) tensor indices"""
    from oracle.tflite_fb import Model as OModel
    om = OModel(buf)
    out = []
    ops = om.operators
    for i in range(len(ops) - 2):
        if ops[i].builtin == B.BATCH_MATMUL and ops[i + 1].builtin == 25 and ops[i + 2].builtin == B.BATCH_MATMUL:
            out.append((ops[i].outputs[0], ops[i + 1].outputs[0], ops[i + 2].outputs[0]))
    return out
