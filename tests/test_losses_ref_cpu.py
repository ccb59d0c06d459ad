"""tests/losses_ref.py, the torch restatement of the fused training loss, against the reference: in
float32 it reproduces every term, the total and every gradient of tests/golden/losses.npz (train.py's
block evaluated with the reference's own normalize / estimate_normals / correlation_score by
tests/golden/make_golden_losses.py), and its NaN rules are train.py's, case by case.

Tolerance.  Both sides run the same torch ops in float32 except where the restatement writes out
what the reference calls: binary_cross_entropy (its backward is (c - t) / max(c (1 - c), 1e-12), the
restatement differentiates the two clamped logs) and the [-1, 0, 1] convolution of the spatial gradient
(a subtraction here).  Measured here: the 21 terms and the total are the same bits (difference 0), the
gradients differ by at most 1.52e-7 of a tensor's largest element (the confidences'); the asserted
bound is 4 ulp of fp32 (4.8e-7, relative) for both."""
import os

import numpy as np
import pytest
import torch

import losses_ref as ref

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses.npz")
ULP4 = 4 * 2.0 ** -23


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def unpack(golden):
    d = {k[3:]: v for k, v in golden.items() if k.startswith("in_")}
    g = lambda key: d.get(key)
    outputs = tuple([g(f"{stem}{k}") for k in range(3)]
                    for stem in ("pred_disp", "pred_conf", "disp0_", "disp1_", "conf0_", "conf1_"))
    data = {k: d[k] for k in ("gt", "validgt", "im2_mono", "gt_right", "validgt_right", "im3_mono")}
    args = {k[4:]: v.item() for k, v in golden.items() if k.startswith("arg_")}
    return outputs, data, args


def grad_names(outputs):
    """The fixture's gradient keys in the order of training_loss_and_grads."""
    stems = ("pred_disp", "pred_conf", "disp0_", "disp1_", "conf0_", "conf1_")
    maps = [f"grad_{stems[i]}{k}" for i in (0, 2, 3) for k in range(3) if outputs[i][k] is not None]
    # the confidences follow their maps' order: sequence, left, right
    confs = [f"grad_{stems[i]}{k}" for i in (1, 4, 5) for k in range(3) if outputs[i][k] is not None]
    return maps, confs


def term_names(outputs):
    """[(block, rows)]: per call the fixture's term keys of each map (L1, N, BCE)."""
    rows = []
    for tag, di in (("seq", 0), ("left", 2), ("right", 3)):
        rows.append([[f"term_{tag}_{t}_{k}" for t in ("l1", "n", "bce")] for k in range(3) if outputs[di][k] is not None])
    return rows


def test_fixture_inputs_are_the_seeded_ones(golden):
    left, right = ref.make_case(2, 9, 33, 6, seed=2024), ref.make_case(2, 9, 33, 3, seed=2025)
    ref.check_case(left), ref.check_case(right)
    assert np.array_equal(golden["in_gt"], left["gt"]) and np.array_equal(golden["in_gt_right"], right["gt"])
    assert np.array_equal(golden["in_pred_disp1"], -left["signs"][1] * left["maps"][1])
    assert np.array_equal(golden["in_disp1_2"], right["signs"][2] * right["maps"][2])
    assert golden["arg_use_normal_loss"] and golden["arg_use_normal_loss_on_coarse"] and golden["arg_use_border_mask"]


def test_float32_restatement_reproduces_the_reference(golden):
    outputs, data, args = unpack(golden)
    total, terms, gmaps, gconfs = ref.training_loss_and_grads(outputs, data, args, torch.float32)
    worst_t = abs(total - float(golden["total"])) / abs(float(golden["total"]))
    seen = 0
    for block, names in zip(terms, term_names(outputs)):
        for row, keys in zip(block, names):
            for v, key in zip(row, keys):
                if key in golden:
                    worst_t = max(worst_t, abs(v - float(golden[key])) / abs(float(golden[key])))
                    seen += 1
                else:
                    assert v == 0.0, key
    assert seen == sum(k.startswith("term_") for k in golden) == 21
    worst_g = 0.0
    mnames, cnames = grad_names(outputs)
    assert len(mnames) == len(gmaps) == 9 and len(cnames) == len(gconfs) == 5
    for g, key in zip(gmaps + gconfs, mnames + cnames):
        want = golden[key].astype(np.float64)
        assert np.abs(want).max() > 0, key
        worst_g = max(worst_g, np.abs(g - want).max() / np.abs(want).max())
    print(f"terms and total: worst relative difference {worst_t:.3g}; gradients: {worst_g:.3g} of max|g|")
    assert worst_t <= ULP4 and worst_g <= ULP4


# ------------------------------------------------------------------- the drop / propagate table
def _case():
    c = ref.make_case(2, 5, 7, 2, seed=7)
    target = ref.estimate_normals(torch.from_numpy(c["mono"]), 0.7).numpy()
    return c, target


def _run(c, target, maps, border="left", **kw):
    return ref.loss_and_grads(maps, c["gt"], c["valid"], c["maxdisp"], target, 0.7, border, 1.0, torch.float32, **kw)


def _seq(c, **kw):
    return ref.Map(c["maps"][0], None, sign=-1, w_l1=0.7, w_n=1.3, **kw)


def _coarse(c, k=1, side="left", **kw):
    return ref.Map(c["maps"][k], c["confs"][k], sign=1, sel=ref.SEL_MASK_BORDER, w_l1=1.0, w_n=10.0, w_bce=1.0,
                   skip_if_nan_map=True, drop_nan_l1=True, drop_nan_bce=side == "right", **kw)


def test_empty_mask_propagates_through_the_iterative_l1():
    c, target = _case()
    c["valid"][:] = 0
    total, terms, gm, _ = _run(c, target, [_seq(c)])
    assert np.isnan(total) and np.isnan(terms[0, 0]) and np.isnan(terms[0, 1])   # (299; the N term is dropped)
    assert not gm[0].any()


def test_empty_border_selection_drops_the_coarse_l1_and_normals():
    c, target = _case()
    c["gt"][:] = 6.5   # col - gt >= 0 nowhere on 7 columns, the mask itself is not empty
    c["maxdisp"] = 9.0
    total, terms, gm, gc = _run(c, target, [_coarse(c)])
    assert np.isnan(terms[0, 0]) and np.isnan(terms[0, 1]) and np.isfinite(terms[0, 2])   # (334, 330)
    assert total == pytest.approx(terms[0, 2]) and not gm[0].any() and gc[0].any()


def test_nan_coarse_map_is_skipped():
    c, target = _case()
    c["maps"][1][1, 0, 2, 3] = np.nan
    total, terms, gm, gc = _run(c, target, [_coarse(c, 1), ref.Map(c["maps"][0], sign=-1, w_l1=0.7)])
    assert not terms[0].any() and not gm[0].any() and not gc[0].any()   # (322)
    assert np.isfinite(total) and total == pytest.approx(0.7 * terms[1, 0], rel=1e-6)


def test_nan_confidences():
    c, target = _case()
    c["confs"][1][:] = np.nan   # every pixel excluded: the BCE is a mean of nothing
    left, _, gm, gc = _run(c, target, [_coarse(c, side="left")])
    assert np.isnan(left) and not gm[0].any() and not gc[0].any()       # (344): propagates; zeros
    right, terms, gm, gc = _run(c, target, [_coarse(c, side="right")], border="right")
    assert np.isfinite(right) and np.isnan(terms[0, 2]) and gm[0].any() and not gc[0].any()   # (376): dropped
    c["confs"][1][:] = 0.5
    c["confs"][1][0, 0, 1, 1] = np.nan   # one pixel: excluded from the mean (340), the rest counts
    total, terms, _, gc = _run(c, target, [_coarse(c)])
    assert np.isfinite(total) and np.isfinite(terms[0, 2]) and gc[0][0, 0, 1, 1] == 0


def test_clip_has_no_slope_at_or_beyond_its_ends():
    c, target = _case()
    conf = c["confs"][1]
    conf[0, 0, 0, :4] = [0.0, 1.0, -0.5, 1.5]
    c["valid"][0, 0, 0, :4] = 1
    c["gt"][0, 0, 0, :4] = 0.5
    total, _, _, gc = _run(c, target, [_coarse(c)])
    assert np.isfinite(total) and not gc[0][0, 0, 0, :4].any() and gc[0][0, 0, 1:].any()
