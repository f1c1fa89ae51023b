"""The reference run of a model: run_reference walks it op by op, the only such
loop of the tests.  An op the oracle does not restate goes to the numpy
evaluator of the family that owns it (TABLE); every other op goes through
OracleInterpreter.run(feed, ops=[i]).  An expected value never comes from the
product.

The family modules hold the evaluators (they are the restatements) and must not
import this module at module level: it imports them."""
import numpy as np

from tests import bmm_models as B
from tests import encoder_models as E
from tests import grouped_models as G
from tests import reindex_models as R

# (claims(om, o) -> bool, evaluate(om, o, vals) -> [arrays]); the claims are disjoint
TABLE = [
    (G.is_grouped, G.eval_grouped),                                   # CONV_2D whose filter has icg != ic, 8-bit
    (lambda om, o: o.builtin in R.REINDEX_OPS, R.eval_reindex),       # TRANSPOSE, slicing, SPLIT, depth / space
    (lambda om, o: o.builtin == B.BATCH_MATMUL, B.eval_bmm),          # int8 and float32
    (E.is_encoder_op, E.eval_encoder_op),                             # 8-bit last-axis MEAN, SQUARED_DIFFERENCE, RSQRT, GELU
]


def claimants(om, o, table=TABLE):
    """indices of the table entries that claim operator o"""
    return [k for k, (claims, _) in enumerate(table) if claims(om, o)]


def run_reference(model_bytes, inputs, table=TABLE):
    """{tensor: value} of every tensor of the model for inputs {tensor: array}
    (or one array for a single-input model)"""
    from oracle.runner import OracleInterpreter
    from oracle.tflite_fb import Model as OModel
    om = OModel(model_bytes)
    interp = OracleInterpreter(om)
    if not isinstance(inputs, dict):
        inputs = {om.inputs[0]: inputs}
    vals = {t.index: t.data for t in om.tensors if t.is_const}
    for k, v in inputs.items():
        vals[k] = np.asarray(v, om.tensors[k].np_dtype).reshape(om.tensors[k].shape)
    for i, o in enumerate(om.operators):
        who = claimants(om, o, table)
        assert len(who) <= 1, "op %d (builtin %d) is claimed by entries %s" % (i, o.builtin, who)
        if who:
            outs = table[who[0]][1](om, o, vals)
            for t, v in zip(o.outputs, outs):
                assert list(v.shape) == om.tensors[t].shape, (o.builtin, v.shape, om.tensors[t].shape)
        else:
            feed = {k: vals[k] for k in o.inputs if k >= 0 and not om.tensors[k].is_const}
            res = interp.run(feed, ops=[i])
            outs = [res[t] for t in o.outputs]
        for t, v in zip(o.outputs, outs):
            vals[t] = np.ascontiguousarray(v).reshape(om.tensors[t].shape)
    return vals
