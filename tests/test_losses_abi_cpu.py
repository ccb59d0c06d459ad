"""The fused training loss's entry points (csrc/losses.hip) without a GPU: the header, the ctypes
table and the library carry them, SaLossMap has one size on both sides, the ABI version is unchanged,
and every refusal is made before any HIP call, returns SA_E_ARG (-1) and leaves a message that names
the limit."""
import ctypes
import re

import pytest

from stereoanywhere_amd import _native as N

# any non-null value: validation fails before a pointer is used
PTR = 64
NEW = ("sa_loss_terms_ws_size", "sa_loss_terms_rec_size", "sa_loss_terms_forward", "sa_loss_terms_backward")


def test_symbols_struct_and_version():
    header = re.sub(r"/\*.*?\*/", "", open(N.HEADER).read(), flags=re.S)
    lib = N.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in N.SIGNATURES and hasattr(lib, name), name
    assert "#define SA_ABI_VERSION 9" in header
    assert N.ABI_VERSION == 9 and lib.sa_abi_version() == 9
    assert "SA_STRUCT_LOSS_MAP = 4" in header and "#define SA_LOSS_MAX_MAPS 32" in header
    assert lib.sa_struct_size(4) == ctypes.sizeof(N.SaLossMap) == 72
    fields = re.search(r"typedef struct \{(.*?)\} SaLossMap;", header, flags=re.S).group(1)
    names = re.findall(r"(\w+)\s*[;,]", fields)
    assert names == [f[0] for f in N.SaLossMap._fields_]


def test_sizes():
    lib = N.lib()
    # (2 + 4 K) doubles per 64 x 16 tile and sample, plus 8 slices x 4 floats per (map, sample)
    assert lib.sa_loss_terms_ws_size(3, 2, 9, 33) == (2 + 12) * 8 * 2 + 3 * 2 * 8 * 4 * 4
    assert lib.sa_loss_terms_ws_size(50, 4, 544, 960) == (2 + 200) * 8 * (15 * 34 * 4) + 50 * 4 * 8 * 4 * 4
    assert lib.sa_loss_terms_rec_size(3, 2) == 8 * (4 + 8 * 3 + 2 * 3 * 2)
    for bad in ((0, 2, 9, 33), (3, 0, 9, 33), (3, 2, 0, 33), (3, 2, 9, 0), (4097, 2, 9, 33)):
        assert lib.sa_loss_terms_ws_size(*bad) == -1
    assert lib.sa_loss_terms_rec_size(0, 2) == -1 and lib.sa_loss_terms_rec_size(3, 0) == -1


def _maps(n=1, **kw):
    arr = (N.SaLossMap * n)()
    for i in range(n):
        f = dict(map=PTR, conf=PTR, grad_map=PTR, grad_conf=PTR, w_l1=1.0, w_n=1.0, w_bce=1.0, sign=1, sel=0, flags=0)
        f.update(kw)
        for k, v in f.items():
            setattr(arr[i], k, v)
    return arr


def _fwd(K=1, maps=None, gt=PTR, valid=PTR, target=PTR, B=1, H=4, W=4, border=0, ws=PTR, rec=PTR, out=PTR, **kw):
    maps = _maps(max(K, 1), **kw) if maps is None else maps
    return N.lib().sa_loss_terms_forward(K, maps, gt, valid, target, B, H, W, 192.0, border, 1.0, 1.0, ws, rec, out, None)


def _bwd(K=1, gt=PTR, valid=PTR, target=PTR, B=1, H=4, W=4, border=0, rec=PTR, g=PTR, **kw):
    return N.lib().sa_loss_terms_backward(K, _maps(max(K, 1), **kw), gt, valid, target, B, H, W, 192.0, border, 1.0,
                                          1.0, rec, g, None)


def _refused(rc, message):
    assert rc == -1
    assert message in N.lib().sa_last_error(), N.lib().sa_last_error()


@pytest.mark.parametrize("call,who", [(_fwd, b"sa_loss_terms_forward"), (_bwd, b"sa_loss_terms_backward")])
def test_common_refusals(call, who):
    for K in (0, -1, 4097):
        _refused(call(K=K), who + b": K must be 1..4096")
    for kw in ({"gt": None}, {"valid": None}, {"rec": None}):
        _refused(call(**kw), who + b": null pointer (maps / gt / valid / rec)")
    for kw in ({"B": 0}, {"H": 0}, {"W": -3}, {"B": 65536}):
        _refused(call(**kw), b"bad shape")
    for border in (-1, 3):
        _refused(call(border=border), b"border_mode must be 0 (none), 1 (left) or 2 (right)")
    _refused(call(rec=PTR + 4), b"rec not 8-byte aligned")
    _refused(call(map=None), b"null pointer (map 0)")
    for sign in (0, 2, -2):
        _refused(call(sign=sign), b"sign must be -1 or +1")
    _refused(call(sel=2), b"sel must be 0 (mask) or 1 (mask and border)")
    _refused(call(flags=8), b"unknown flags")
    _refused(call(w_n=float("nan")), b"a weight is NaN")
    _refused(call(target=None), b"has a normals weight but target is null")
    _refused(call(conf=None, grad_conf=None), b"has a BCE weight but no confidence")
    # the second map is checked too
    _refused(call(K=2, sign=3), b"map 0: sign")


def test_forward_and_backward_refusals():
    _refused(N.lib().sa_loss_terms_forward(1, None, PTR, PTR, PTR, 1, 4, 4, 192.0, 0, 1.0, 1.0, PTR, PTR, PTR, None),
             b"null pointer (maps / gt / valid / rec)")
    for kw in ({"ws": None}, {"out": None}):
        _refused(_fwd(**kw), b"sa_loss_terms_forward: null pointer (ws / out)")
    _refused(_fwd(ws=PTR + 4), b"workspace not 8-byte aligned")
    _refused(_bwd(g=None), b"sa_loss_terms_backward: null pointer (g_total)")
    _refused(_bwd(grad_map=None, grad_conf=None), b"null pointer (no gradient requested)")
    _refused(_bwd(conf=None, w_bce=0.0), b"grad_conf requested without conf")
    with pytest.raises(N.NativeError, match="K must be 1..4096"):
        N.call("sa_loss_terms_backward", 0, None, None, None, None, 1, 1, 1, 1.0, 0, 1.0, 1.0, None, None, None)
