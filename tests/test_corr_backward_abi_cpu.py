"""Argument validation of the three backward entry points (corr_backward.hip) without a GPU: every
refusal is made before any HIP call, returns SA_E_ARG (-1) and leaves a message."""
import pytest

from stereoanywhere_amd import _native as N

# any non-null value: validation fails before a pointer is used
PTR = 64


def _lookup(go=PTR, cx=PTR, gp=PTR, W2=48, L=4, R=4, rs=92):
    return N.lib().sa_corr_lookup_backward(go, L * (2 * R + 1) * 6, cx, 6, 1, 2, 3, W2, L, R, gp, rs, None)


def test_abi_version():
    assert N.ABI_VERSION == 9 and N.lib().sa_abi_version() == 9


@pytest.mark.parametrize("null", ["grad_out", "coords_x", "grad_pyramid"])
def test_lookup_backward_null(null):
    args = {"go": PTR, "cx": PTR, "gp": PTR}
    args[{"grad_out": "go", "coords_x": "cx", "grad_pyramid": "gp"}[null]] = None
    assert _lookup(**args) == -1
    assert b"sa_corr_lookup_backward: null pointer" in N.lib().sa_last_error()


def test_lookup_backward_domain():
    lib = N.lib()
    assert _lookup(L=5, rs=200) == -1
    assert b"num_levels must be 1..4" in lib.sa_last_error()
    assert _lookup(L=0) == -1
    assert b"num_levels must be 1..4" in lib.sa_last_error()
    assert _lookup(R=17) == -1
    assert b"radius must be 0..16" in lib.sa_last_error()
    assert _lookup(R=-1) == -1
    assert b"radius must be 0..16" in lib.sa_last_error()
    # widths 8, 4, 2, 1: the coarsest level cannot be sampled
    assert _lookup(W2=8, rs=16) == -1
    assert b"too narrow" in lib.sa_last_error()
    # 48 + 24 + 12 + 6 = 90 floats per row
    assert _lookup(rs=88) == -1
    assert b"row_stride" in lib.sa_last_error()


def test_pyramid_backward_refusals():
    lib = N.lib()
    assert lib.sa_corr_pyramid_backward(None, 4, 48, 92, 4, PTR, 48, None) == -1
    assert b"sa_corr_pyramid_backward: null pointer" in lib.sa_last_error()
    assert lib.sa_corr_pyramid_backward(PTR, 4, 48, 92, 4, None, 48, None) == -1
    assert b"sa_corr_pyramid_backward: null pointer" in lib.sa_last_error()
    assert lib.sa_corr_pyramid_backward(PTR, 4, 48, 200, 5, PTR, 48, None) == -1
    assert b"num_levels must be 1..4" in lib.sa_last_error()
    assert lib.sa_corr_pyramid_backward(PTR, 4, 48, 92, 4, PTR, 47, None) == -1
    assert b"bad shape" in lib.sa_last_error()
    assert lib.sa_corr_pyramid_backward(PTR, 4, 48, 88, 4, PTR, 48, None) == -1
    assert b"row_stride too small" in lib.sa_last_error()


def test_volume_backward_refusals():
    lib = N.lib()

    def run(G=PTR, f2=PTR, f3=PTR, g2=PTR, g3=PTR, C=8, vrs=48):
        return lib.sa_corr_volume_backward(G, vrs, f2, f3, 1, C, 2, 40, 48, 2.0, g2, g3, None)
    for kw in ({"G": None}, {"f2": None}, {"f3": None}, {"g2": None, "g3": None}):
        assert run(**kw) == -1
        assert b"sa_corr_volume_backward: null pointer" in lib.sa_last_error()
    assert run(C=0) == -1
    assert b"empty shape" in lib.sa_last_error()
    assert run(vrs=47) == -1
    assert b"row stride too small" in lib.sa_last_error()
    with pytest.raises(N.NativeError, match="null pointer"):
        N.call("sa_corr_volume_backward", None, 48, PTR, PTR, 1, 8, 2, 40, 48, 2.0, PTR, PTR, None)
