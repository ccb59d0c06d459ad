"""The volume stage's entry points (csrc/volume_stage.hip) without a GPU: the header, the derived
ctypes table and the library carry them, the ABI version and the timing-id count are unchanged, and
every refusal is made before any HIP call, returns SA_E_ARG (-1) and leaves a message that names the
limit."""
import re

import pytest

from stereoanywhere_amd import _native as N

# any non-null values: validation fails before a pointer is used
PTR, OUT = 1 << 20, 1 << 30
NEW = ("sa_volume_peak", "sa_volume_stage", "sa_volume_truncate_backward")
NONE, ROLL, NOISE, ZERO = 0, 1, 2, 3


def test_symbols_constants_and_version():
    header = re.sub(r"/\*.*?\*/", "", open(N.HEADER).read(), flags=re.S)
    lib = N.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
        assert name in N.SIGNATURES and hasattr(lib, name), name
    assert "#define SA_ABI_VERSION 9" in header
    assert N.ABI_VERSION == 9 and lib.sa_abi_version() == 9
    assert N.CONST["SA_K_COUNT"] == 20   # the new launches are timed under SA_K_MISC
    assert [N.CONST["SA_VOLAUG_" + k] for k in ("NONE", "ROLL", "NOISE", "ZERO")] == [NONE, ROLL, NOISE, ZERO]


def test_derived_signatures():
    P, I, L, F = N.P, N.I, N.L, N.F
    assert N.SIGNATURES["sa_volume_peak"] == (I, [P, L, P, P, L, P])
    assert N.SIGNATURES["sa_volume_stage"] == (I, [P, I, I, I, I, I, P, I, I, I, P, P, P, P, F, P, P])
    assert N.SIGNATURES["sa_volume_truncate_backward"] == (I, [P, I, I, I, I, P, P, F, P, P])
    assert N.lib().sa_volume_stage.argtypes == N.SIGNATURES["sa_volume_stage"][1]


def _stage(volume=PTR, B=1, H=2, W1=8, W2=8, kind=NONE, mde=PTR, nbins=4, bin=0, shift=1, noise=PTR, peak=PTR,
           disp=None, conf=None, out=OUT):
    return N.lib().sa_volume_stage(volume, B, H, W1, W2, kind, mde, nbins, bin, shift, noise, peak, disp, conf, 0.9,
                                   out, None)


def _bwd(g=PTR, B=1, H=2, W1=8, W2=8, disp=PTR, conf=PTR, out=OUT):
    return N.lib().sa_volume_truncate_backward(g, B, H, W1, W2, disp, conf, 0.9, out, None)


def _refused(rc, message):
    assert rc == -1
    assert message in N.lib().sa_last_error(), N.lib().sa_last_error()


def test_stage_refusals():
    for kw in ({"volume": None}, {"out": None}):
        _refused(_stage(**kw), b"sa_volume_stage: null pointer (volume / out)")
    for kw in ({"B": 0}, {"H": -1}, {"W1": 0}, {"W2": 0}):
        _refused(_stage(**kw), b"sa_volume_stage: bad shape")
    _refused(_stage(B=1 << 15, H=1 << 15, W1=4, W2=4), b"rows exceed 2^31 - 1")
    for kind in (-1, 4):
        _refused(_stage(kind=kind), b"kind must be SA_VOLAUG_NONE, _ROLL, _NOISE or _ZERO")
    _refused(_stage(disp=PTR), b"trunc_disp and trunc_conf go together")
    _refused(_stage(conf=PTR), b"trunc_disp and trunc_conf go together")
    for kind in (ROLL, NOISE, ZERO):
        _refused(_stage(kind=kind, mde=None), b"null pointer (mde, needed by every augmentation)")
        for nbins in (0, 65):
            _refused(_stage(kind=kind, nbins=nbins), b"nbins must be 1..64")
        for b in (-1, 4):
            _refused(_stage(kind=kind, bin=b), b"bin must be 0..nbins-1")
    for shift in (0, -1, 9):
        _refused(_stage(kind=ROLL, shift=shift), b"shift must be 1..W1")
    _refused(_stage(kind=ROLL, out=PTR), b"SA_VOLAUG_ROLL cannot run in place")
    _refused(_stage(kind=ROLL, out=PTR + 4 * 100), b"SA_VOLAUG_ROLL cannot run in place")   # a partial overlap
    _refused(_stage(kind=NOISE, noise=None), b"null pointer (noise, needed by SA_VOLAUG_NOISE)")
    _refused(_stage(kind=ZERO, peak=None), b"null pointer (peak, needed by SA_VOLAUG_ZERO)")
    _refused(_stage(kind=ZERO, W2=12), b"SA_VOLAUG_ZERO needs W1 == W2")
    _refused(_stage(disp=PTR, conf=PTR, W2=12), b"the truncation needs W1 == W2")
    # what a kind does not read may be null: the refusal that follows is the next check's
    _refused(_stage(kind=NONE, mde=None, noise=None, peak=None, nbins=0, bin=9, shift=0, out=None),
             b"null pointer (volume / out)")


def test_peak_and_backward_refusals():
    lib = N.lib()
    for args in ((None, 8, PTR, PTR, 4), (PTR, 8, None, PTR, 4), (PTR, 8, PTR, None, 4)):
        _refused(lib.sa_volume_peak(*args, None), b"sa_volume_peak: null pointer (volume / peak / work)")
    for count in (0, -4):
        _refused(lib.sa_volume_peak(PTR, count, PTR, PTR, 4, None), b"count must be positive")
    _refused(lib.sa_volume_peak(PTR, 8, PTR, PTR, 0, None), b"work_floats must be positive")
    for kw in ({"g": None}, {"disp": None}, {"conf": None}, {"out": None}):
        _refused(_bwd(**kw), b"sa_volume_truncate_backward: null pointer")
    for kw in ({"B": 0}, {"W1": -2}):
        _refused(_bwd(**kw), b"sa_volume_truncate_backward: bad shape")
    _refused(_bwd(W2=9), b"the truncation needs W1 == W2")
    with pytest.raises(N.NativeError, match="shift must be 1..W1"):
        N.call("sa_volume_stage", PTR, 1, 2, 8, 8, ROLL, PTR, 4, 0, 0, None, None, None, None, 0.9, OUT, None)
