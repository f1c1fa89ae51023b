"""The conv / depthwise launchers' routing is host logic (no device call) and a
pure function of the params struct.  Every expected name below was recorded
from the library of the commit before the environment knobs were retired
(default environment), so the table pins that routing did not move; the
BH_CONV_ROWS hint is new and follows include/band_hip_kernels.h.  Pointers are
16-byte-aligned placeholders, never dereferenced.
"""
import ctypes

import pytest

from band_amd import _abi

BATCHES = (1, 24, 32, 256)

DIRECT, STEM, STEM_LDS, STEM_MFMA = ("conv_direct_kernel", "conv_stem_kernel", "conv_stem_lds_kernel",
                                     "conv_stem_mfma_kernel")
XS, ROWS, MFMA, GEMM, BIG = ("conv_xs_kernel", "conv_rows_kernel", "conv_mfma_kernel", "conv_gemm_kernel",
                             "conv_gemm_big_kernel")
DW_RUN, DW_DOT, DW_TAP, DW_MFMA, DW_GENERIC = ("dwconv3x3_run_kernel", "dwconv3x3_dot_kernel", "dwconv3x3_kernel",
                                               "dwconv3x3_mfma_kernel", "dwconv_generic_kernel")


def same_pad(size, k, stride):
    out = (size + stride - 1) // stride
    return out, max(0, ((out - 1) * stride + k - size) // 2)


def conv_name(lib, b, hw, ic, oc, k=1, stride=1, hint=0, in_xor=0, w_zp=0):
    out, pad = same_pad(hw, k, stride)
    p = _abi.ConvParams(batch=b, in_h=hw, in_w=hw, in_c=ic, out_h=out, out_w=out, out_c=oc, k_h=k, k_w=k,
                        stride_h=stride, stride_w=stride, dil_h=1, dil_w=1, pad_h=pad, pad_w=pad,
                        k_pad=(k * k * ic + 63) // 64 * 64, n_pad=(oc + 63) // 64 * 64, in_xor=in_xor, w_zp=w_zp,
                        kernel_hint=hint)
    p.input, p.output, p.weights = 1 << 20, 2 << 20, 3 << 20
    return lib.bh_conv2d_i8_kernel(ctypes.byref(p)).decode()


def dw_name(lib, b, hw, ch, k=3, stride=1, hint=0):
    out, pad = same_pad(hw, k, stride)
    p = _abi.DwConvParams(batch=b, in_h=hw, in_w=hw, in_c=ch, out_h=out, out_w=out, out_c=ch, depth_multiplier=1,
                          k_h=k, k_w=k, stride_h=stride, stride_w=stride, dil_h=1, dil_w=1, pad_h=pad, pad_w=pad,
                          kernel_hint=hint)
    p.input, p.output, p.weights = 1 << 20, 2 << 20, 3 << 20
    p.taps = (4 << 20) if k == 3 else 0  # the tap table of the 3x3 forms
    return lib.bh_dwconv2d_i8_kernel(ctypes.byref(p)).decode()


# (spatial, in_c, out_c) -> names at BATCHES: tests/kernel_harness.py's MNV2_POINTWISE
POINTWISE = {
    (112, 32, 16): (XS, XS, XS, XS),
    (112, 16, 96): (XS, XS, XS, XS),
    (56, 96, 24): (XS, XS, XS, XS),
    (56, 24, 144): (XS, XS, XS, XS),
    (56, 144, 24): (XS, XS, XS, XS),
    (28, 144, 32): (MFMA, XS, XS, XS),
    (28, 32, 192): (MFMA, XS, XS, XS),
    (28, 192, 32): (MFMA, XS, XS, XS),
    (14, 192, 64): (MFMA, XS, XS, XS),
    (14, 64, 384): (MFMA, XS, XS, XS),
    (14, 384, 64): (MFMA, MFMA, MFMA, GEMM),
    (14, 384, 96): (MFMA, MFMA, MFMA, GEMM),
    (14, 96, 576): (MFMA, XS, XS, XS),
    (14, 576, 96): (MFMA, MFMA, MFMA, GEMM),
    (7, 576, 160): (MFMA, MFMA, MFMA, GEMM),
    (7, 160, 960): (MFMA, MFMA, MFMA, BIG),
    (7, 960, 160): (MFMA, MFMA, MFMA, GEMM),
    (7, 960, 320): (MFMA, MFMA, MFMA, GEMM),
    (7, 320, 1280): (MFMA, MFMA, GEMM, BIG),
    (1, 1280, 1001): (MFMA, MFMA, MFMA, MFMA),
}

# (batch, spatial, in_c, out_c, in_xor) -> name: the layers of test_conv1x1_rows_batched
# (0x80: uint8) and test_conv1x1_gemm_vs_mfma in tests/test_kernels_gpu.py
BATCHED_1X1 = {
    (4, 112, 16, 96, 0x00): XS,
    (4, 112, 32, 16, 0x80): XS,
    (12, 56, 24, 144, 0x00): XS,
    (12, 56, 144, 24, 0x80): XS,
    (44, 28, 32, 192, 0x00): XS,
    (44, 28, 192, 32, 0x00): XS,
    (170, 14, 64, 384, 0x00): XS,
    (170, 14, 96, 20, 0x80): XS,
    (700, 7, 64, 520, 0x00): XS,
    (700, 7, 40, 1004, 0x00): XS,
    (45, 28, 12, 72, 0x80): XS,
    (6, 14, 512, 1024, 0x00): GEMM,
    (24, 14, 960, 160, 0x00): GEMM,
    (8, 7, 1280, 546, 0x00): MFMA,
    (6, 14, 576, 273, 0x00): MFMA,
    (1, 14, 16, 24, 0x00): MFMA,
    (3, 9, 48, 20, 0x00): MFMA,
    (6, 14, 1024, 17, 0x00): MFMA,
    (2, 7, 160, 960, 0x00): MFMA,
    (24, 7, 320, 1280, 0x00): MFMA,
    (5, 13, 96, 64, 0x00): MFMA,
    (24, 14, 512, 1024, 0x00): GEMM,
    (24, 14, 192, 1000, 0x00): XS,
}

# (spatial, in_c, out_c, stride) -> names at BATCHES: 3x3 layers
CONV3X3 = {
    (224, 3, 32, 1): (STEM_MFMA, STEM_MFMA, STEM_MFMA, STEM_MFMA),
    (224, 3, 32, 2): (STEM_MFMA, STEM_MFMA, STEM_MFMA, STEM_MFMA),
    (56, 16, 64, 1): (MFMA, MFMA, MFMA, MFMA),
    (56, 16, 64, 2): (MFMA, MFMA, MFMA, MFMA),
    (28, 64, 64, 1): (MFMA, MFMA, MFMA, MFMA),
    (28, 64, 64, 2): (MFMA, MFMA, MFMA, MFMA),
}

# (spatial, channels, stride) -> names at BATCHES: MobileNetV2's 3x3 depthwise layers
DEPTHWISE = {
    (112, 32, 1): (DW_DOT, DW_RUN, DW_RUN, DW_RUN),
    (112, 96, 2): (DW_DOT, DW_RUN, DW_RUN, DW_RUN),
    (56, 144, 1): (DW_DOT, DW_RUN, DW_RUN, DW_RUN),
    (56, 144, 2): (DW_DOT, DW_RUN, DW_RUN, DW_RUN),
    (28, 192, 1): (DW_DOT, DW_RUN, DW_RUN, DW_RUN),
    (28, 192, 2): (DW_DOT, DW_RUN, DW_RUN, DW_RUN),
    (14, 384, 1): (DW_DOT, DW_RUN, DW_RUN, DW_RUN),
    (14, 576, 1): (DW_DOT, DW_RUN, DW_RUN, DW_RUN),
    (14, 576, 2): (DW_DOT, DW_RUN, DW_RUN, DW_RUN),
    (7, 960, 1): (DW_DOT, DW_RUN, DW_RUN, DW_RUN),
}

# hint -> ((eligible layer, name), (ineligible layer, name)); layers are
# conv_name's (b, hw, ic, oc, k, stride, in_xor).  An ineligible layer keeps
# the name it has without a hint.
STEM32 = (32, 224, 3, 32, 3, 2, 0x80)
SMALL_1X1 = (1, 14, 96, 576, 1, 1, 0)
CONV_HINTS = {
    1: (((24, 14, 960, 160, 1, 1, 0), MFMA), (STEM32, STEM_MFMA)),
    2: ((SMALL_1X1, GEMM), ((1, 14, 96, 576, 1, 1, 0x80), MFMA)),
    3: ((SMALL_1X1, BIG), ((1, 14, 96, 576, 1, 1, 0x80), MFMA)),
    4: ((STEM32, STEM_LDS), (SMALL_1X1, MFMA)),
    5: ((STEM32, STEM_MFMA), ((32, 224, 3, 24, 3, 2, 0x80), STEM_LDS)),
    6: ((STEM32, STEM), (SMALL_1X1, MFMA)),
    7: (((24, 14, 960, 160, 1, 1, 0), ROWS), ((1, 1, 1280, 1001, 1, 1, 0), MFMA)),
}
# hint -> ((eligible layer, name), (ineligible layer, name)); dw_name's (b, hw, ch, k, stride)
DW_HINTS = {
    1: (((1, 14, 384, 3, 1), DW_RUN), ((1, 14, 96, 5, 1), DW_GENERIC)),
    2: (((24, 56, 144, 3, 1), DW_DOT), ((1, 14, 96, 5, 1), DW_GENERIC)),
    3: (((24, 14, 384, 3, 1), DW_MFMA), ((24, 14, 36, 3, 1), DW_DOT)),
}


@pytest.fixture(scope="module")
def lib():
    return _abi.load()


def check_all(lib):
    for (hw, ic, oc), names in POINTWISE.items():
        for b, want in zip(BATCHES, names):
            assert conv_name(lib, b, hw, ic, oc) == want, (b, hw, ic, oc)
    for (b, hw, ic, oc, in_xor), want in BATCHED_1X1.items():
        assert conv_name(lib, b, hw, ic, oc, in_xor=in_xor, w_zp=5 if in_xor else 0) == want, (b, hw, ic, oc)
    for (hw, ic, oc, stride), names in CONV3X3.items():
        for b, want in zip(BATCHES, names):
            assert conv_name(lib, b, hw, ic, oc, k=3, stride=stride) == want, (b, hw, ic, oc, stride)
    for (hw, ch, stride), names in DEPTHWISE.items():
        for b, want in zip(BATCHES, names):
            assert dw_name(lib, b, hw, ch, stride=stride) == want, (b, hw, ch, stride)


def test_default_routes(lib):
    check_all(lib)
    # one uint8 layer, one asymmetric-filter layer (int8 and symmetric: GEMM
    # above), one 5x5 depthwise layer
    assert conv_name(lib, 24, 14, 960, 160, in_xor=0x80) == MFMA
    assert conv_name(lib, 24, 14, 960, 160, w_zp=3) == MFMA
    assert dw_name(lib, 24, 14, 96, k=5) == DW_GENERIC


def test_hints(lib):
    for hint, ((layer, forced), (other, fallen)) in CONV_HINTS.items():
        b, hw, ic, oc, k, stride, in_xor = layer
        assert conv_name(lib, b, hw, ic, oc, k, stride, hint, in_xor) == forced, hint
        b, hw, ic, oc, k, stride, in_xor = other
        assert conv_name(lib, b, hw, ic, oc, k, stride, hint, in_xor) == fallen, hint
        assert conv_name(lib, b, hw, ic, oc, k, stride, 0, in_xor) == fallen, hint
    for hint, ((layer, forced), (other, fallen)) in DW_HINTS.items():
        assert dw_name(lib, *layer, hint=hint) == forced, hint
        assert dw_name(lib, *other, hint=hint) == fallen, hint
        assert dw_name(lib, *other, hint=0) == fallen, hint


def test_routing_ignores_the_environment(lib, monkeypatch):
    """the retired knobs' names, at values that moved routes before"""
    monkeypatch.setenv("BH_CONV_ROWS_MIN_M", "0")
    monkeypatch.setenv("BH_CONV_GEMM", "0")
    monkeypatch.setenv("BH_GEMM_BIG_CFG", "1")
    check_all(lib)
    assert lib.bh_conv_gemm_big_config(256 * 49, 1280) == 3
