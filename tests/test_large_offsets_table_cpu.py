"""Completeness of the far-stride table (tests/large_offsets_util.py) against the C ABI's header, without a
GPU: every `long` stride parameter of include/stereoanywhere_hip.h has a row, the table names nothing the
header does not have, and a parameter the table lists as gated is refused before any launch: a new entry
point cannot be added without its row."""
import pytest

import large_offsets_util as U
from stereoanywhere_amd import _native as N


def test_the_parameter_list_is_the_headers():
    params = U.header_stride_params()
    assert len(params) == len(set(params)) > 90
    # the families the list must hold, one of each naming form
    for key in (("sa_gru_zr", "c_bs"), ("sa_corr_lookup", "coords_bstride"), ("sa_corr_volume_pyramid", "row_stride"),
                ("sa_tile_stitch", "disp_ts"), ("sa_softargmin_conf", "sk"), ("SaWinoProblem", "skip_bs"),
                ("SaGateEpilogue", "head_part_bs"), ("SaResampleJob", "in_bs"), ("SaFeatureGateJob", "out_bs"),
                ("sa_conv_direct_close", "out_ds_bs")):
        assert key in params, key
    # counts and sizes are not strides
    for key in (("sa_corr_pyramid_from_volume", "rows"), ("sa_norm_act", "hw"), ("sa_volume_peak", "count")):
        assert key not in params, key
    assert not [f for f, _ in N.SaLossMap._fields_ if ("SaLossMap", f) in params], "SaLossMap has no strides"


def test_every_stride_parameter_has_a_row():
    missing = [k for k in U.header_stride_params() if k not in U.TABLE]
    assert not missing, f"no far-stride row, gate or open entry for {missing}"
    stale = [k for k in U.TABLE if k not in U.header_stride_params()]
    assert not stale, f"the table names parameters the header does not have: {stale}"


def test_a_missing_row_is_noticed():
    """The check above fails when a row is taken out."""
    key = ("sa_relu_copy", "in_bs")
    saved = U.TABLE.pop(key)
    try:
        with pytest.raises(AssertionError, match="sa_relu_copy"):
            test_every_stride_parameter_has_a_row()
    finally:
        U.TABLE[key] = saved
    header = open(N.HEADER).read().replace("int sa_relu_copy(const float *in, long in_bs",
                                           "int sa_relu_copy(const float *in, long in_bs, long mask2_bs")
    assert ("sa_relu_copy", "mask2_bs") in U.header_stride_params(header)   # a new parameter shows up in the list


def test_rows_cover_what_the_table_says():
    for key, (kind, what) in U.TABLE.items():
        if kind == "far":
            owner, params, _ = U.FAR_ROWS[what]
            assert (key[1] in params and owner == key[0]) or ".".join(key) in params, (key, what)
        else:
            assert kind == "gated" and key in U.GATED and U.GATED[key][0] == what, key
    for name, (owner, params, _) in U.FAR_ROWS.items():
        for q in params:
            key = tuple(q.split(".")) if "." in q else (owner, q)
            assert key in U.header_stride_params(), f"row {name}: {key[0]} has no parameter {key[1]}"


@pytest.mark.parametrize("key", sorted(U.GATED), ids=lambda k: f"{k[0]}.{k[1]}")
def test_gated_parameters_refuse_the_far_stride(key):
    where, call, message = U.GATED[key]
    path, line = where.rsplit(":", 1)
    src = open(f"{N.ROOT}/{path}").read().splitlines()
    assert "SA_REQUIRE" in src[int(line) - 1] and key[1] in src[int(line) - 1], f"{where} is not {key[1]}'s gate"
    assert call() == -1   # SA_E_ARG: refused before any HIP call
    assert message in N.lib().sa_last_error(), N.lib().sa_last_error()
