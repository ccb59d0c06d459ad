"""The up-cat conv's backward entry points (csrc/upcat_backward.hip) without a GPU: the header, the derived
ctypes table and the library carry them, the ABI version and the timing-id count are unchanged, the
work-size query gives its documented count, and every refusal is made before any HIP call, returns SA_E_ARG
(-1) and leaves a message that names the limit."""
import re

import pytest

from stereoanywhere_amd import _native as N

# any non-null values: validation fails before a pointer is used
X, G, W, OUT, DW, WORK = 1 << 20, 1 << 24, 1 << 28, 1 << 30, 1 << 34, 1 << 36
NEW = ("sa_trilinear_up_adjoint", "sa_conv3d_pointwise_backward_work", "sa_conv3d_pointwise_backward")
BUILT = {(8, 8): 1, (16, 16): 4, (16, 8): 2, (32, 16): 4}   # (Cx, Cg): slices S of the Cx rows


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
    P, I, L = N.P, N.I, N.L
    assert N.SIGNATURES["sa_trilinear_up_adjoint"] == (I, [P, I, I, I, I, I, I, I, I, P, P])
    assert N.SIGNATURES["sa_conv3d_pointwise_backward_work"] == (L, [I, I, I, L])
    assert N.SIGNATURES["sa_conv3d_pointwise_backward"] == (I, [P, P, P, I, I, I, L, P, P, P, P])
    assert N.lib().sa_conv3d_pointwise_backward.argtypes == N.SIGNATURES["sa_conv3d_pointwise_backward"][1]


def test_work_size_query():
    """B ceil(n / 16384) blocks of 4 waves, Cx Cg / S float64 sums per wave."""
    work = N.lib().sa_conv3d_pointwise_backward_work
    for (cx, cg), s in BUILT.items():
        per_block = 4 * (cx * cg // s)
        assert work(cx, cg, 1, 1) == per_block
        assert work(cx, cg, 1, 16384) == per_block and work(cx, cg, 1, 16385) == 2 * per_block
        assert work(cx, cg, 4, 240 * 136 * 240) == 4 * -(-240 * 136 * 240 // 16384) * per_block
        assert work(cx, cg, 0, 8) == -1 and work(cx, cg, 1, 0) == -1
    for pair in ((8, 16), (4, 4), (32, 32), (0, 0)):
        assert work(*pair, 1, 8) == -1


def _refused(rc, message):
    assert rc == -1
    assert message in N.lib().sa_last_error(), N.lib().sa_last_error()


def _adj(g=G, B=1, C=8, D=4, H=6, W_=8, Dp=2, Hp=3, Wp=4, dp=OUT):
    return N.lib().sa_trilinear_up_adjoint(g, B, C, D, H, W_, Dp, Hp, Wp, dp, None)


def _bwd(x=X, g=G, w=W, Cx=8, Cg=8, B=1, n=64, work=WORK, dx=OUT, dw=DW):
    return N.lib().sa_conv3d_pointwise_backward(x, g, w, Cx, Cg, B, n, work, dx, dw, None)


def test_adjoint_refusals():
    for kw in ({"g": None}, {"dp": None}):
        _refused(_adj(**kw), b"sa_trilinear_up_adjoint: null pointer (g / dp)")
    for kw in ({"B": 0}, {"C": -1}, {"D": 1}, {"H": 1}, {"W_": 0}, {"Dp": 0}, {"Hp": -2}, {"Wp": 0}):
        _refused(_adj(**kw), b"sa_trilinear_up_adjoint: bad shape")
    _refused(_adj(D=1), b"D, H, W at least 2")
    for kw in ({"Dp": 3}, {"Hp": 4}, {"Wp": 5}):   # 2 (n - 1) > N - 1
        _refused(_adj(**kw), b"at most half size")
    _refused(_adj(D=1 << 11, H=1 << 10, W_=1 << 10), b"must be below 2^31")
    _refused(_adj(B=1 << 15, C=1 << 15, D=4, H=9, W_=2, Dp=2, Hp=5, Wp=1), b"blocks exceed 2^31 - 1")
    _refused(_adj(dp=G), b"dp overlaps g")
    _refused(_adj(dp=G + 4 * 100), b"dp overlaps g")   # a partial overlap
    with pytest.raises(N.NativeError, match="at most half size"):
        N.call("sa_trilinear_up_adjoint", G, 1, 8, 2, 2, 2, 2, 1, 1, OUT, None)


def test_backward_refusals():
    for kw in ({"x": None}, {"g": None}, {"w": None}):
        _refused(_bwd(**kw), b"sa_conv3d_pointwise_backward: null pointer (x / g / w)")
    for kw in ({"B": 0}, {"n": 0}, {"n": -5}):
        _refused(_bwd(**kw), b"sa_conv3d_pointwise_backward: bad shape")
    _refused(_bwd(n=1 << 31), b"must be below 2^31")
    _refused(_bwd(dx=None, dw=None), b"no output")
    _refused(_bwd(work=None), b"dw needs work")
    assert _bwd(work=None, dw=None, Cx=8, Cg=16) == -1   # work is not needed without dw: the next refusal
    for pair in ((8, 16), (4, 4), (32, 32)):
        _refused(_bwd(Cx=pair[0], Cg=pair[1]), b"no kernel built for %d x %d" % pair)
    _refused(_bwd(B=1 << 20, n=(1 << 31) - 1), b"blocks exceed 2^31 - 1")
    for dx in (X, G, W, X + 4 * 8 * 64 - 4):
        _refused(_bwd(dx=dx), b"dx overlaps x, g or w")
    for dw in (X, G, W + 4 * 63):
        _refused(_bwd(dw=dw), b"dw overlaps x, g or w")
    with pytest.raises(N.NativeError, match="no kernel built for 8 x 16"):
        N.call("sa_conv3d_pointwise_backward", X, G, W, 8, 16, 1, 64, WORK, OUT, DW, None)


def test_forward_dispatch_names_its_instances():
    """sa_conv3d_pointwise_upcat refuses an unbuilt pair as before (the <16, 16, identity a> instance that
    training uses is exercised on the GPU)."""
    rc = N.lib().sa_conv3d_pointwise_upcat(X, 4, None, None, 0, None, None, G, 1, 1, 1, 1, 2, 2, 2, 0.01, W, 4, OUT,
                                           WORK, None)
    _refused(rc, b"sa_conv3d_pointwise_upcat: no kernel built for 4 -> 4")
