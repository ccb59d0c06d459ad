"""The 3x3x3 conv backward's entry points (csrc/conv3d_backward.hip, sa_conv3d_mf_scaled) without a GPU: the
header, the derived ctypes table and the library carry them, the ABI version and the timing-id count are
unchanged, the work-size query gives its documented count, and every refusal is made before any HIP call,
returns SA_E_ARG (-1) and leaves a message that names the limit."""
import re

import pytest

from stereoanywhere_amd import _native as N

# any non-null values: validation fails before a pointer is used
X, G, TAB, OUT, DW, WORK, SC = 1 << 20, 1 << 30, 1 << 36, 1 << 38, 1 << 40, 1 << 42, 1 << 44
NEW = ("sa_sample_scale", "sa_conv3d_mf_scaled", "sa_conv3d_k3_backward_weight_work", "sa_conv3d_k3_backward_weight")


def test_symbols_and_version():
    header = re.sub(r"/\*.*?\*/", "", open(N.HEADER).read(), flags=re.S)
    lib = N.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in N.SIGNATURES and hasattr(lib, name), name
    assert "#define SA_ABI_VERSION 9" in header
    assert N.ABI_VERSION == 9 and lib.sa_abi_version() == 9
    assert N.CONST["SA_K_COUNT"] == 20   # the new launches are timed under SA_K_MISC


def test_derived_signatures():
    P, I, L, F = N.P, N.I, N.L, N.F
    assert N.SIGNATURES["sa_sample_scale"] == (I, [P, I, L, I, P, P, P, P])
    assert N.SIGNATURES["sa_conv3d_k3_backward_weight_work"] == (L, [I, I, I, I, I])
    assert N.SIGNATURES["sa_conv3d_k3_backward_weight"] == (I, [P, P, I, I, I, I, I, P, P, P, P, P])
    mf = N.SIGNATURES["sa_conv3d_mf"]
    assert N.SIGNATURES["sa_conv3d_mf_scaled"] == (I, mf[1][:11] + [P] + mf[1][11:]) and mf[1][10] == F


def test_work_size_query():
    """One block per sample, 4 x 64 (C = 32: 4 x 32) tile of (h, w) and range of planes; 27 C C doubles each."""
    work = N.lib().sa_conv3d_k3_backward_weight_work
    assert N.lib().sa_conv3d_mf_get_planes() == 0
    for C, tw in ((8, 64), (16, 64), (32, 32)):
        per = 27 * C * C
        assert work(C, 1, 1, 1, 1) == per
        assert work(C, 3, 8, 4, tw) == 3 * per and work(C, 3, 8, 5, tw + 1) == 3 * 4 * per
        # planes are halved while the grid holds fewer than 512 blocks and a block more than 8 planes
        assert work(C, 1, 64, 4, tw) == 8 * per
        for bad in ((C, 0, 4, 4, 4), (C, 1, 0, 4, 4), (C, 1, 4, -1, 4), (C, 1, 4, 4, 0)):
            assert work(*bad) == -1
    N.lib().sa_conv3d_mf_set_planes(3)
    try:
        assert work(16, 2, 7, 5, 66) == 2 * 3 * 2 * 2 * 27 * 256   # the forward's override cuts D here too
    finally:
        N.lib().sa_conv3d_mf_set_planes(0)
    for C in (4, 12, 64, 0):
        assert work(C, 1, 4, 4, 4) == -1
    assert work(8, 4, 240, 136, 240) == 4 * 34 * 4 * 27 * 64 and work(16, 4, 120, 68, 120) == 4 * 4 * 17 * 2 * 27 * 256


def _refused(rc, message):
    assert rc == -1
    assert message in N.lib().sa_last_error(), N.lib().sa_last_error()


def _scale(t=X, B=2, n=64, rep=8, state=WORK, scale=SC, inv=OUT):
    return N.lib().sa_sample_scale(t, B, n, rep, state, scale, inv, None)


def _dw(x=X, g=G, C=8, B=1, D=4, H=4, W=8, xs=None, gs=SC, work=WORK, dw=DW):
    return N.lib().sa_conv3d_k3_backward_weight(x, g, C, B, D, H, W, xs, gs, work, dw, None)


def _mf(inp=X, B=1, C=8, D=4, H=4, W=8, table=TAB, Cout=8, mean=SC, rstd=SC + 4096, slope=1.0, osc=SC + 8192, out=OUT):
    return N.lib().sa_conv3d_mf_scaled(inp, B, C, D, H, W, table, Cout, mean, rstd, slope, osc, out, None, None)


def test_sample_scale_refusals():
    for kw in ({"t": None}, {"state": None}, {"scale": None}, {"inv": None}):
        _refused(_scale(**kw), b"sa_sample_scale: null pointer (t / state / scale / inv)")
    for kw in ({"B": 0}, {"B": 65536}, {"n": 0}, {"rep": 0}):
        _refused(_scale(**kw), b"sa_sample_scale: bad shape")
    _refused(_scale(B=65536), b"(1 .. 65535)")


def test_backward_weight_refusals():
    for kw in ({"x": None}, {"g": None}, {"work": None}, {"dw": None}):
        _refused(_dw(**kw), b"sa_conv3d_k3_backward_weight: null pointer (x / g / work / dw)")
    for kw in ({"B": 0}, {"D": 0}, {"H": -1}, {"W": 0}):
        _refused(_dw(**kw), b"sa_conv3d_k3_backward_weight: bad shape")
    for C in (4, 12, 64):
        _refused(_dw(C=C), b"no kernel built for %d -> %d channels (built: 8 -> 8, 16 -> 16, 32 -> 32)" % (C, C))
    _refused(_dw(D=1 << 10, H=1 << 10, W=1 << 10), b"must be below 2^30")
    for dw in (X, G + 4 * 100, WORK):
        _refused(_dw(dw=dw), b"dw overlaps x, g or work")
    for work in (X, G + 8):
        _refused(_dw(work=work), b"work overlaps x or g")
    with pytest.raises(N.NativeError, match="no kernel built for 12 -> 12"):
        N.call("sa_conv3d_k3_backward_weight", X, G, 12, 1, 4, 4, 8, None, SC, WORK, DW, None)


def test_scaled_forward_refusals():
    _refused(_mf(osc=None), b"sa_conv3d_mf_scaled: null pointer (out_scale)")
    _refused(_mf(inp=None), b"sa_conv3d_mf: null pointer")
    _refused(_mf(C=8, Cout=16), b"built for 8 -> 8, 16 -> 16 and 32 -> 32")
    _refused(_mf(D=1 << 10, H=1 << 10, W=1 << 10), b"< 2^30 voxels")
    _refused(_mf(C=32, Cout=32, D=1 << 9, H=1 << 9, W=1 << 6), b"< 2^31 bytes")
