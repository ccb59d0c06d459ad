"""The fused training loss (csrc/losses.hip) through ops.loss_terms / ops.loss_terms_backward, against
torch.autograd of its restatement in float64 (tests/losses_ref.py) from the same fp32 inputs.

The yardstick is the one of tests/test_gpu_lsq_lrc_backward.py: with e_ref = max |fp32 torch - fp64|
of the restatement on the CPU (asserted > 0: the seeds are chosen so), every gradient tensor, every
term and the total must satisfy max |hip - fp64| <= 4 e_ref.  Every case runs twice: the same bits.

Inputs are losses_ref.make_case: away from the kinks for all pixels (check_case asserts it, and no
pixel is left out of any comparison).  B = 2 with different mn / mx per sample; map 0's second sample
is a constant plane (mx = mn).

Tiles: the forward kernel's block owns 64 x 16 pixels (width x height), the backward's 64 x 4; 19 x 70
spans two tiles of either in each direction.  1 x 2 and 2 x 1: every stencil index clamps."""
import functools

import numpy as np
import pytest
import torch

import losses_ref as ref
from stereoanywhere_amd import ops

pytestmark = pytest.mark.gpu
dev = "cuda"

SHAPES = [(1, 2), (2, 1), (5, 7), (9, 33), (3, 65), (19, 70)]
B = 2
UP = 0.37   # the upstream scalar
# 1000 H + W unless listed: with 2001 (and 2003) the pixels of 2 x 1 give an L1 term that fp32 computes exactly (e_ref = 0)
SEEDS = {(2, 1): 2005}

# (w_l1, w_n, w_bce) of the three maps per case
WEIGHTS = {"l1": [(0.7, 0, 0), (1.0, 0, 0), (0.9, 0, 0)],
           "n": [(0, 1.3, 0), (0, 10.0, 0), (0, 0.4, 0)],
           "bce": [(0, 0, 0.6), (0, 0, 1.0), (0, 0, 0.8)],
           "all": [(0.7, 1.3, 0.6), (1.0, 10.0, 1.0), (0.9, 0.4, 0.8)]}


def g(a):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)


def c(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def same_bits(a, b):
    if a is None or b is None:
        return a is None and b is None
    i = torch.int64 if a.dtype == torch.float64 else torch.int32
    return torch.equal(a.view(i), b.view(i))


def border_of(W):
    """left where a column can pass col - gt >= 0 with gt >= 0.05 (W > 1), else right"""
    return "left" if W > 1 else "right"


def specs(case, weights):
    """K ref.Maps over make_case's maps: sign from the case, the selection and the flags cycling."""
    out = []
    for k, (m, cf, s) in enumerate(zip(case["maps"], case["confs"], case["signs"])):
        w1, wn, wb = weights[k % len(weights)] if k < 3 else tuple(
            w * (1 + 0.01 * k) if (k + i) % 4 else 0.0 for i, w in enumerate(weights[k % len(weights)]))
        coarse = k % 3 == 1
        out.append(ref.Map(m, cf if (wb != 0 or k % 2) else None, sign=s,
                           sel=ref.SEL_MASK_BORDER if coarse else ref.SEL_MASK, w_l1=w1, w_n=wn, w_bce=wb,
                           skip_if_nan_map=coarse, drop_nan_l1=coarse, drop_nan_bce=k % 3 == 2))
    return out


def hip_maps(maps):
    return [ops.LossMap(g(M.map), g(M.conf), M.sign, M.sel, M.w_l1, M.w_n, M.w_bce,
                        (ops.LOSS_SKIP_IF_NAN_MAP if M.skip_if_nan_map else 0)
                        | (ops.LOSS_DROP_NAN_L1 if M.drop_nan_l1 else 0)
                        | (ops.LOSS_DROP_NAN_BCE if M.drop_nan_bce else 0)) for M in maps]


@functools.lru_cache(maxsize=None)
def problem(H, W, which, K=3, seed=None):
    case = ref.make_case(B, H, W, K, seed=SEEDS.get((H, W), 1000 * H + W) if seed is None else seed)
    ref.check_case(case)
    gain = W / 10
    target = ref.estimate_normals(torch.from_numpy(case["mono"]), gain).numpy()
    maps = specs(case, WEIGHTS[which])
    kw = dict(gt=case["gt"], valid=case["valid"], maxdisp=case["maxdisp"], target=target, gain=gain,
              border=border_of(W), lrc_th=1.0)
    return maps, kw


@functools.lru_cache(maxsize=None)
def reference(H, W, which, K=3, seed=None):
    maps, kw = problem(H, W, which, K, seed)
    return (ref.loss_and_grads(maps, dtype=torch.float64, upstream=UP, **kw),
            ref.loss_and_grads(maps, dtype=torch.float32, upstream=UP, **kw))


def run_hip(maps, kw, need_map=None, need_conf=None):
    hm = hip_maps(maps)
    args = (g(kw["gt"]), g(kw["valid"]), kw["maxdisp"], g(kw["target"]), kw["gain"], kw["border"], kw["lrc_th"])
    out, rec = ops.loss_terms(hm, *args)
    if need_conf is None:
        need_conf = [M.conf is not None for M in maps]
    gm, gc = ops.loss_terms_backward(hm, *args, rec, torch.tensor([UP], device=dev), need_map, need_conf)
    return out, rec, gm, gc


def compare(label, got, want64, want32, worst=None):
    """max |got - fp64| <= 4 e_ref, e_ref > 0."""
    got, want64, want32 = (np.asarray(a, dtype=np.float64) for a in (got, want64, want32))
    e_ref = np.abs(want32 - want64).max()
    err = np.abs(got - want64).max()
    print(f"{label}: err {err:.3g}, e_ref {e_ref:.3g}, err/e_ref {err / e_ref if e_ref else float('inf'):.3g}")
    if worst is not None:
        worst.append(err / e_ref if e_ref else float("inf"))
    assert np.isfinite(want64).all() and e_ref > 0, label + ": e_ref is 0 (pick another seed)"
    assert np.isfinite(got).all(), label
    assert err <= 4 * e_ref, label


def check_all(label, maps, hip, hip2, want64, want32):
    out, rec, gm, gc = hip
    for a, b in zip([out, rec] + gm + gc, [hip2[0], hip2[1]] + hip2[2] + hip2[3]):
        assert same_bits(a, b), label + ": two runs differ"
    t64, terms64, gm64, gc64 = want64
    t32, terms32, gm32, gc32 = want32
    o = c(out)
    worst = []
    compare(f"{label} total", o[0], t64, t32, worst)
    terms = o[1:].reshape(-1, 3)
    for k, M in enumerate(maps):
        for j, (name, w) in enumerate((("L1", M.w_l1), ("N", M.w_n), ("BCE", M.w_bce))):
            if w == 0:
                assert terms[k, j] == 0, f"{label} {name}_{k}"
            else:
                compare(f"{label} {name}_{k}", terms[k, j], terms64[k, j], terms32[k, j], worst)
        if M.w_l1 != 0 or M.w_n != 0:
            compare(f"{label} grad_map_{k}", c(gm[k]), gm64[k], gm32[k], worst)
        else:
            assert not c(gm[k]).any() and not gm64[k].any()
        if M.conf is not None and M.w_bce != 0:
            compare(f"{label} grad_conf_{k}", c(gc[k]), gc64[k], gc32[k], worst)
        elif M.conf is not None:
            assert not c(gc[k]).any() and not gc64[k].any()
    print(f"{label}: worst err / e_ref {max(worst):.3g}")


@pytest.mark.parametrize("which", list(WEIGHTS))
@pytest.mark.parametrize("H,W", SHAPES)
def test_terms_and_gradients(H, W, which):
    """Every term alone and all together, K = 3: a sign -1 map over mask, a skip-if-NaN map over
    mask and border, a sign +1 map over mask."""
    maps, kw = problem(H, W, which)
    want64, want32 = reference(H, W, which)
    check_all(f"{H}x{W} {which}", maps, run_hip(maps, kw), run_hip(maps, kw), want64, want32)


@pytest.mark.parametrize("K", [1, 35])
def test_map_counts(K):
    """K = 1, and K = 35: two launches (32 + 3) into one partial-sum buffer, mixed signs, selections,
    weights, maps without some terms and without confidences."""
    maps, kw = problem(5, 7, "all", K)
    want64, want32 = reference(5, 7, "all", K)
    if K == 35:
        assert {M.sign for M in maps} == {-1, 1} and {M.sel for M in maps} == {0, 1}
        assert any(M.w_l1 == 0 for M in maps[32:]) and any(M.w_bce == 0 for M in maps[32:]) and all(M.w_n for M in maps[32:])
        assert any(M.conf is None for M in maps) and any(M.w_l1 == 0 for M in maps)
    check_all(f"K={K}", maps, run_hip(maps, kw), run_hip(maps, kw), want64, want32)


def test_need_subsets():
    """An output that is not asked for is None; the others keep their bits."""
    maps, kw = problem(9, 33, "all")
    _, _, gm, gc = run_hip(maps, kw)
    for need_map, need_conf in (([True, False, False], [False, False, False]),
                                ([False, False, False], [False, True, False]),
                                ([False, True, True], [True, False, True]),
                                ([False, False, True], [False, False, False])):
        _, _, pm, pc = run_hip(maps, kw, need_map, need_conf)
        for n, a, b in zip(need_map + need_conf, pm + pc, gm + gc):
            assert (a is None) if not n else torch.equal(a, b)
    with pytest.raises(RuntimeError, match="nothing to compute"):
        run_hip(maps, kw, [False] * 3, [False] * 3)


def test_record():
    """The record: counts, live coefficients w / count, mn / mx per (map, sample); map 0's second sample
    is the constant plane."""
    maps, kw = problem(9, 33, "all")
    _, rec, _, _ = run_hip(maps, kw)
    r = c(rec)
    gt, valid = (torch.from_numpy(kw[k]) for k in ("gt", "valid"))
    mask, mask_b = ref.selections(gt, valid, kw["maxdisp"], kw["border"])
    assert r.shape == (4 + 8 * 3 + 2 * 3 * B,) and r[1] == 0
    assert r[2] == int(mask.sum()) and r[3] == int(mask_b.sum()) and 0 < r[3] < r[2]
    for k, M in enumerate(maps):
        R = r[4 + 8 * k: 12 + 8 * k]
        cnt = r[3] if M.sel else r[2]
        assert R[0] == 0 and R[7] == r[2]
        assert np.array_equal(R[1:4], [M.w_l1 / cnt, M.w_n / cnt, M.w_bce / r[2]])
        x = M.sign * M.map.astype(np.float64)
        mm = r[4 + 8 * 3 + 2 * B * k:][:2 * B].reshape(B, 2)
        assert np.array_equal(mm[:, 0], x.min((1, 2, 3))) and np.array_equal(mm[:, 1], x.max((1, 2, 3)))
    mm0 = r[4 + 8 * 3:][:2 * B].reshape(B, 2)
    assert mm0[1, 0] == mm0[1, 1] and mm0[0, 0] < mm0[0, 1]


# --------------------------------------------------------------------------- the NaN table
def nan_problem(kind):
    case = ref.make_case(B, 5, 7, 3, seed=77)
    gain = 0.7
    border = "left"
    if kind.startswith("empty mask"):
        case["valid"][:] = 0
        border = "right"
    elif kind == "empty border":
        case["gt"][:] = 6.5
        case["maxdisp"] = 9.0
    elif kind == "nan coarse map":
        case["maps"][1][1, 0, 2, 3] = np.nan
    elif kind == "nan confidences":
        case["confs"][1][:] = np.nan
        border = "right"
    elif kind == "nan total":
        case["confs"][1][:] = np.nan   # the left-side BCE propagates
    elif kind == "nan iterative map":
        case["maps"][0][0, 0, 1, 2] = np.nan
        case["valid"][0, 0, 1, 2], case["gt"][0, 0, 1, 2] = 1, 0.5   # inside the mask
    target = ref.estimate_normals(torch.from_numpy(case["mono"]), gain).numpy()
    maps = specs(case, WEIGHTS["all"])
    maps[1].drop_nan_bce = border == "right"
    if kind == "empty mask, coarse":
        maps = maps[1:2]   # every term of the right-side coarse map is dropped: the total is 0
    return maps, dict(gt=case["gt"], valid=case["valid"], maxdisp=case["maxdisp"], target=target, gain=gain,
                      border=border, lrc_th=1.0)


NAN_TOTAL = ("empty mask, iterative", "nan total", "nan iterative map")


@pytest.mark.parametrize("kind", ["empty mask, coarse", "empty mask, iterative", "empty border", "nan coarse map", "nan confidences", "nan total",
                                  "nan iterative map"])
def test_nan_rules(kind):
    """Each row of the drop / propagate table against the restatement: the same terms are NaN, the
    total is NaN or not as there, dropped terms and skipped maps get exact zeros, a NaN total gives
    all-zero gradients, and whatever stays finite is within 4 e_ref (where e_ref > 0) of float64."""
    maps, kw = nan_problem(kind)
    t64, terms64, gm64, gc64 = ref.loss_and_grads(maps, dtype=torch.float64, upstream=UP, **kw)
    t32, terms32, gm32, gc32 = ref.loss_and_grads(maps, dtype=torch.float32, upstream=UP, **kw)
    hip, hip2 = run_hip(maps, kw), run_hip(maps, kw)
    out, rec, gm, gc = hip
    for a, b in zip([out, rec] + gm + gc, [hip2[0], hip2[1]] + hip2[2] + hip2[3]):
        assert same_bits(a, b), kind + ": two runs differ"
    o = c(out)
    assert np.isnan(o[0]) == np.isnan(t64), kind
    assert np.isnan(t64) == (kind in NAN_TOTAL)
    assert np.array_equal(np.isnan(o[1:].reshape(-1, 3)), np.isnan(terms64)), kind
    assert c(rec)[1] == float(np.isnan(t64))
    if not np.isnan(t64):
        e = abs(t32 - t64)
        assert abs(o[0] - t64) <= (4 * e if e > 0 else 2.0 ** -24 * abs(t64))
    for k, M in enumerate(maps):
        for got, w64, w32 in ((gm[k], gm64[k], gm32[k]), (gc[k], gc64[k], gc32[k])):
            if got is None:
                continue
            got = c(got)
            assert np.isfinite(got).all() and np.isfinite(w64).all()
            if not w64.any():
                assert not got.any(), f"{kind}: map {k}"
            else:
                e = np.abs(w32 - w64).max()
                assert e > 0 and np.abs(got - w64).max() <= 4 * e, f"{kind}: map {k}"
    if kind in NAN_TOTAL:
        assert all(not c(t).any() for t in gm + gc if t is not None)
    if kind == "nan coarse map":
        assert c(rec)[4 + 8] == 1 and not o[1 + 3: 1 + 6].any()
    if kind == "empty mask, coarse":
        assert o[0] == 0 and np.isnan(o[1:4]).all()
    if kind == "empty border":
        assert np.isnan(o[1 + 3]) and np.isnan(o[1 + 4]) and np.isfinite(o[1 + 5])


def test_clip_ends_get_exact_zeros():
    """Confidences outside [0, 1] and exactly 0 and 1: zero gradient there, the rest as the restatement."""
    maps, kw = problem(5, 7, "bce", 3, 4242)
    maps = [ref.Map(**M.__dict__) for M in maps]
    odd = np.array([0.0, 1.0, -0.5, 1.5], dtype=np.float32)
    kw = dict(kw, valid=kw["valid"].copy())
    mask = ref.selections(torch.from_numpy(kw["gt"]), torch.from_numpy(kw["valid"]), kw["maxdisp"], "none")[0]
    at = np.flatnonzero(mask.numpy())[:4]   # four pixels inside the mask
    for M in maps:
        M.conf = M.conf.copy()
        M.conf.reshape(-1)[at] = odd
    want64 = ref.loss_and_grads(maps, dtype=torch.float64, upstream=UP, **kw)
    want32 = ref.loss_and_grads(maps, dtype=torch.float32, upstream=UP, **kw)
    out, rec, gm, gc = run_hip(maps, kw)
    compare("clip total", c(out)[0], want64[0], want32[0])
    for k in range(3):
        got = c(gc[k])
        assert not got.reshape(-1)[at].any() and not want64[3][k].reshape(-1)[at].any()
        assert (got.reshape(-1)[np.flatnonzero(mask.numpy())[4:]] != 0).all()
        compare(f"clip grad_conf_{k}", got, want64[3][k], want32[3][k])


def test_refusals():
    maps, kw = problem(5, 7, "all")
    hm = hip_maps(maps)
    args = [g(kw["gt"]), g(kw["valid"]), kw["maxdisp"], g(kw["target"]), kw["gain"], kw["border"], kw["lrc_th"]]
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        ops.loss_terms(hm, args[0].cpu(), *args[1:])
    with pytest.raises(RuntimeError, match="must be float32"):
        ops.loss_terms([hm[0]._replace(map=hm[0].map.half())], *args)
    with pytest.raises(RuntimeError, match="must have gt's shape"):
        ops.loss_terms([hm[0]._replace(map=hm[0].map[:, :, :, :5].contiguous())], *args)
    with pytest.raises(RuntimeError, match="no target normals"):
        ops.loss_terms(hm, *args[:3], None, *args[4:])
    with pytest.raises(RuntimeError, match="BCE weight but no confidence"):
        ops.loss_terms([hm[0]._replace(conf=None)], *args)
    with pytest.raises(RuntimeError, match="border must be one of"):
        ops.loss_terms(hm, *args[:5], "top", 1.0)
    with pytest.raises(ops.N.NativeError, match="sign must be -1 or \\+1"):
        ops.loss_terms([hm[0]._replace(sign=2)], *args)
    out, rec = ops.loss_terms(hm, *args)
    with pytest.raises(RuntimeError, match="rec must be the contiguous float64 GPU record"):
        ops.loss_terms_backward(hm, *args, rec[:-1], torch.ones(1, device=dev))
    with pytest.raises(RuntimeError, match="g_total must hold one float"):
        ops.loss_terms_backward(hm, *args, rec, torch.ones(2, device=dev))
