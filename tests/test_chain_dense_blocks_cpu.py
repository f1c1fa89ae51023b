"""The dense chain form's interior blocks, counted on the host: dense_blocks()
of tests/test_chain_dense_gpu.py (every pixel of a 16-pixel block exists and
has all nine taps inside the image) on the shapes that file runs.  The four
shapes the form was first tested on have no interior block; each INTERIOR shape
has the counts worked out by hand below, and blocks on both sides of the rule.
"""
import numpy as np

from tests.test_chain_dense_gpu import CASES, INTERIOR, NARROW, dense_blocks, make_case

# (b, h, w, stride, dilation) -> (non-empty blocks, interior blocks)
#   1x3x33:   P = 99; row 1, ox 1 .. 31 is m 34 .. 64: block 3 (m 48 .. 63) alone
#   1x6x35:   P = 210; rows 1 .. 4, ox 1 .. 33: one block per row (m 36 .. 68 holds 48 .. 63, ...)
#   2x5x21:   P = 210; rows 1 .. 3, ox 1 .. 19 hold a whole block once per image
#   1x5x67/2: 3 x 34 outputs, P = 102; row 1, ox 1 .. 32 (m 35 .. 66): block 3
#   1x7x37 d2: pad 2; rows 2 .. 4, ox 2 .. 34: one block per row
COUNTS = {(1, 3, 33, 1, 1): (7, 1), (1, 6, 35, 1, 1): (14, 4), (2, 5, 21, 1, 1): (14, 2), (1, 5, 67, 2, 1): (7, 1),
          (1, 7, 37, 1, 2): (17, 3)}
EARLIER = {(1, 5, 7, 1, 1): 3, (3, 9, 13, 1, 1): 22, (1, 11, 10, 2, 1): 2, (2, 14, 14, 1, 2): 25}


def _key(a):
    return (a["b"], a["h"], a["w"], a["stride"], a.get("dil", 1))


def test_interior_shapes_have_the_counted_blocks():
    assert {_key(a) for a in INTERIOR} == set(COUNTS)
    for a in INTERIOR:
        interior = dense_blocks(make_case(a))
        assert (len(interior), int(interior.sum())) == COUNTS[_key(a)], _key(a)
        assert interior.any() and not interior.all()
    assert np.flatnonzero(dense_blocks(make_case(INTERIOR[0]))).tolist() == [3]
    # 2x5x21: one interior block in each image (105 pixels per image)
    two = np.flatnonzero(dense_blocks(make_case(INTERIOR[2]))) * 16
    assert (two // 105).tolist() == [0, 1] and ((two + 15) // 105).tolist() == [0, 1]


def test_earlier_shapes_have_no_interior_block():
    assert {_key(a) for a in CASES + NARROW} == set(EARLIER)
    for a in CASES + NARROW:
        interior = dense_blocks(make_case(a))
        assert len(interior) == EARLIER[_key(a)], _key(a)
        assert not interior.any(), _key(a)


def test_interior_cases_cover_what_they_claim():
    """1 and 3 channel groups, residual with a stored first output, no second
    1x1, both requantisation forms, the input zero point at -128 and inside"""
    assert {a["ce"] for a in INTERIOR} >= {16, 48}
    assert any(a["residual"] and a.get("store_pw1") and a["ce2"] for a in INTERIOR)
    assert any(a["ce2"] == 0 for a in INTERIOR)
    assert {a.get("fast", True) for a in INTERIOR} == {True, False}
    assert any(a["e_zp"] == -128 for a in INTERIOR) and any(-128 < a["e_zp"] < 127 for a in INTERIOR)
    assert {a["cout"] for a in NARROW} >= {4, 12, 20} and any(a["ce2"] == 20 for a in NARROW)
