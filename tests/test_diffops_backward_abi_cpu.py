"""The backward entry points of soft-argmin / confidence and convex up-sampling
(csrc/diffops_backward.hip) without a GPU: the header, the ctypes table and the library carry them,
the ABI version is unchanged, and every refusal is made before any HIP call, returns SA_E_ARG (-1)
and leaves a message that names the limit."""
import re

import pytest

from stereoanywhere_amd import _native as N

# any non-null value: validation fails before a pointer is used
PTR = 64
NEW = ("sa_softargmin_conf_backward_ws_size", "sa_softargmin_conf_backward", "sa_convex_upsample_backward")


def test_symbols_and_version():
    header = re.sub(r"/\*.*?\*/", "", open(N.HEADER).read(), flags=re.S)
    lib = N.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in N.SIGNATURES and hasattr(lib, name), name
    assert "#define SA_ABI_VERSION 9" in header
    assert N.ABI_VERSION == 9 and lib.sa_abi_version() == 9


def test_ws_size():
    lib = N.lib()
    # 16 bytes (max, 1 / sum e, fp64 E or S) per strided line and volume: O(B H (W1 + W2))
    assert lib.sa_softargmin_conf_backward_ws_size(4, 136, 240, 240) == 2 * 16 * 4 * 136 * 240
    assert lib.sa_softargmin_conf_backward_ws_size(2, 3, 37, 50) == 2 * 16 * 2 * 3 * 50
    assert lib.sa_softargmin_conf_backward_ws_size(2, 3, 1, 50) == -1
    assert lib.sa_softargmin_conf_backward_ws_size(0, 3, 8, 8) == -1


def _sam(vd=PTR, vc=PTR, g=(PTR, PTR, PTR, PTR), od=PTR, oc=PTR, ws=PTR, W1=8, W2=8, strides=(192, 64, 8, 1), B=1):
    return N.lib().sa_softargmin_conf_backward(vd, vc, B, 3, W1, W2, *strides, *g, od, oc, ws, None)


def test_softargmin_backward_refusals():
    lib = N.lib()
    assert _sam(g=(None, None, None, None)) == -1
    assert b"sa_softargmin_conf_backward: null pointer (all four upstream gradients)" in lib.sa_last_error()
    for kw in ({"vd": None}, {"od": None}):
        assert _sam(**kw) == -1
        assert b"null pointer (vol_disp / grad_vol_disp)" in lib.sa_last_error()
    for kw in ({"vc": None}, {"oc": None}):
        assert _sam(**kw) == -1
        assert b"null pointer (vol_conf / grad_vol_conf)" in lib.sa_last_error()
    # the workspace is required exactly when the strided side has a gradient: the right maps in the
    # reference layout (sk == 1), the left ones in the native layout (sj == 1)
    for kw in ({}, {"g": (PTR, PTR, None, None)}, {"g": (None, None, None, PTR)},
               {"g": (PTR, None, None, None), "strides": (192, 8, 1, 24)}):
        assert _sam(ws=None, **kw) == -1
        assert b"null pointer (workspace" in lib.sa_last_error()
    assert _sam(ws=PTR + 4) == -1
    assert b"8-byte aligned" in lib.sa_last_error()
    assert _sam(W1=1) == -1
    assert b"W1, W2 > 1" in lib.sa_last_error()
    assert _sam(B=0) == -1
    assert b"bad shape" in lib.sa_last_error()
    assert _sam(strides=(192, 64, 8, 2)) == -1
    assert b"one of sj/sk must be 1" in lib.sa_last_error()
    # a volume without an upstream gradient may be null: the call is refused for the other reason only
    assert _sam(vd=None, od=None, g=(None, None, PTR, PTR), W2=1) == -1
    assert b"bad shape" in lib.sa_last_error()
    with pytest.raises(N.NativeError, match="null pointer"):
        N.call("sa_softargmin_conf_backward", None, None, 1, 3, 8, 8, 192, 64, 8, 1, None, None, None, None, None,
               None, None, None)


def _cub(flow=PTR, mask=PTR, go=PTR, gf=PTR, gm=PTR, f=4, mbs=None, B=1, H=2, W=3):
    mbs = 9 * f * f * H * W if mbs is None else mbs
    return N.lib().sa_convex_upsample_backward(flow, mask, mbs, go, B, H, W, f, float(f), gf, gm, None)


def test_convex_backward_refusals():
    lib = N.lib()
    for kw in ({"mask": None}, {"go": None}):
        assert _cub(**kw) == -1
        assert b"sa_convex_upsample_backward: null pointer (mask / grad_out)" in lib.sa_last_error()
    assert _cub(gf=None, gm=None) == -1
    assert b"null pointer (grad_flow and grad_mask)" in lib.sa_last_error()
    assert _cub(flow=None) == -1
    assert b"null pointer (flow" in lib.sa_last_error()
    for f in (9, 0):
        assert _cub(f=f) == -1
        assert b"factor must be 1..8" in lib.sa_last_error()
    assert _cub(H=0) == -1
    assert b"empty shape" in lib.sa_last_error()
    assert _cub(mbs=9 * 16 * 6 - 1) == -1
    assert b"mask batch stride too small" in lib.sa_last_error()
