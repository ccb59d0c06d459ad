"""The volume close's entry points (csrc/volume_close.hip) without a GPU: the header, the derived ctypes
table and the library carry them, the ABI version and the timing-id count are unchanged, the size
queries give the documented counts, and every refusal is made before any HIP call, returns SA_E_ARG
(-1) and leaves a message that names the limit."""
import re

import pytest

from stereoanywhere_amd import _native as N

# any non-null values: validation fails before a pointer is used
PTR, G, OUT, WORK = 1 << 20, 1 << 24, 1 << 30, 1 << 36
NEW = ("sa_volume_close_stat_parts", "sa_volume_close_stats", "sa_volume_close_backward_work",
       "sa_volume_close_backward")


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
    assert N.SIGNATURES["sa_volume_close_stat_parts"] == (L, [I, I, I])
    assert N.SIGNATURES["sa_volume_close_stats"] == (I, [P, I, I, I, I, I, P, P])
    assert N.SIGNATURES["sa_volume_close_backward_work"] == (L, [I, I, I])
    assert N.SIGNATURES["sa_volume_close_backward"] == (I, [P, P, I, I, I, I, I, P, P, P, P, F, P, P, P, P, P])
    assert N.lib().sa_volume_close_backward.argtypes == N.SIGNATURES["sa_volume_close_backward"][1]


def test_size_queries():
    lib = N.lib()
    assert lib.sa_volume_close_stat_parts(1, 2, 3) == 1
    assert lib.sa_volume_close_stat_parts(1, 1, 16384) == 1 and lib.sa_volume_close_stat_parts(1, 1, 16385) == 2
    assert lib.sa_volume_close_stat_parts(240, 136, 240) == -(-240 * 136 * 240 // 16384)
    assert lib.sa_volume_close_backward_work(4, 8, 136) == 2 * 32 * 137
    for bad in ((0, 2, 3), (1, -1, 3), (1, 2, 0)):
        assert lib.sa_volume_close_stat_parts(*bad) == -1
        assert lib.sa_volume_close_backward_work(*bad) == -1


def _refused(rc, message):
    assert rc == -1
    assert message in N.lib().sa_last_error(), N.lib().sa_last_error()


def _stats(x=PTR, B=1, C=2, D=4, H=2, W=8, partial=OUT):
    return N.lib().sa_volume_close_stats(x, B, C, D, H, W, partial, None)


def _bwd(x=PTR, g=G, B=1, C=2, D=4, H=2, W=8, mean=PTR, rstd=PTR, gl=PTR, gr=PTR, work=WORK, dx=OUT, dgl=OUT,
         dgr=OUT):
    return N.lib().sa_volume_close_backward(x, g, B, C, D, H, W, mean, rstd, gl, gr, 0.01, work, dx, dgl, dgr, None)


SHAPE_REFUSALS = (({"B": 0}, b"bad shape"), ({"C": -1}, b"bad shape"), ({"D": 0}, b"bad shape"),
                  ({"H": 0}, b"bad shape"), ({"W": -3}, b"bad shape"),
                  ({"D": 1 << 10, "H": 1 << 10, "W": 1 << 10}, b"must be below 2^30"),
                  ({"D": 1, "H": 1, "W": 1}, b"InstanceNorm needs D*H*W > 1"),
                  ({"B": 1 << 10, "C": 1 << 10, "D": 1 << 10, "H": 1 << 10, "W": 2}, b"rows exceed 2^31 - 1"))


def test_stats_refusals():
    for kw in ({"x": None}, {"partial": None}):
        _refused(_stats(**kw), b"sa_volume_close_stats: null pointer (x / stats_partial)")
    for kw, message in SHAPE_REFUSALS:
        _refused(_stats(**kw), message)
        _refused(_stats(**kw), b"sa_volume_close_stats: bad shape")


def test_backward_refusals():
    for kw in ({"x": None}, {"g": None}, {"mean": None}, {"rstd": None}, {"work": None}):
        _refused(_bwd(**kw), b"sa_volume_close_backward: null pointer (x / grad_out / mean / rstd / work)")
    for kw, message in SHAPE_REFUSALS:
        _refused(_bwd(**kw), message)
        _refused(_bwd(**kw), b"sa_volume_close_backward: bad shape")
    _refused(_bwd(gl=None), b"gate_l and gate_r go together")
    _refused(_bwd(gr=None), b"gate_l and gate_r go together")
    _refused(_bwd(gl=None, gr=None), b"grad_gate_l / grad_gate_r need the gate maps")
    _refused(_bwd(gl=None, gr=None, dgl=None), b"grad_gate_l / grad_gate_r need the gate maps")
    _refused(_bwd(dx=None, dgl=None, dgr=None), b"no output")
    _refused(_bwd(gl=None, gr=None, dx=None, dgl=None, dgr=None), b"no output")
    _refused(_bwd(dx=PTR), b"grad_x overlaps x or grad_out")
    _refused(_bwd(dx=G + 4 * 10), b"grad_x overlaps x or grad_out")   # a partial overlap
    with pytest.raises(N.NativeError, match="InstanceNorm needs"):
        N.call("sa_volume_close_stats", PTR, 1, 1, 1, 1, 1, OUT, None)
