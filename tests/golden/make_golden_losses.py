"""Generate tests/golden/losses.npz by running the REFERENCE's loss here.

Test infrastructure only; run in the build container (where the reference is mounted), never on
the GPU box:

    python tests/golden/make_golden_losses.py

``normalize``, ``estimate_normals`` and ``correlation_score`` are the reference's own
(models/stereoanywhere/utils/utils.py:56-77, 285-293, the functions train.py:32 imports under the same
names), imported through the stubs of tests/golden/make_golden.py (kornia's spatial_gradient is the
restatement there).  The terms of train.py:281-379 are evaluated by the glue below, written for this
file: boolean-mask gathers, ``F.binary_cross_entropy``, the isnan checks, ``sum(all_losses)``, in
float32, followed by torch.autograd for the gradients.

Flags: use_normal_loss, use_normal_loss_on_coarse and use_border_mask on, a right-side ground truth.
B 2, 9 x 33 planes, 3 predictions (the last with a confidence, train.py:308-316) and the three coarse
entries of each side (one without confidence on either side).  The inputs are the seeded ones of
tests/losses_ref.py make_case and are stored as data next to every term, the total and the gradients.
"""
from __future__ import annotations

import math
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import _load_reference  # noqa: E402
import losses_ref  # noqa: E402

ARGS = dict(maxdisp=15.0, lrc_th=1.0, normal_gain=10, use_normal_loss=True, use_normal_loss_on_coarse=True,
            use_border_mask=True)
B, H, W = 2, 9, 33


def inputs():
    left = losses_ref.make_case(B, H, W, 6, seed=2024)
    right = losses_ref.make_case(B, H, W, 3, seed=2025)
    assert left["maxdisp"] == right["maxdisp"] == ARGS["maxdisp"]
    d = dict(gt=left["gt"], validgt=left["valid"], im2_mono=left["mono"], gt_right=right["gt"],
             validgt_right=right["valid"], im3_mono=right["mono"])
    # make_case's sign pattern is -1 for k % 3 == 0; the predictions are -disparity, the coarse maps +
    for k in range(3):
        d[f"pred_disp{k}"] = -left["signs"][k] * left["maps"][k]
        d[f"disp0_{k}"] = left["signs"][3 + k] * left["maps"][3 + k]
        d[f"disp1_{k}"] = right["signs"][k] * right["maps"][k]
    d["pred_conf2"] = left["confs"][2]
    d["conf0_0"], d["conf0_1"] = left["confs"][3], left["confs"][4]
    d["conf1_0"], d["conf1_2"] = right["confs"][0], right["confs"][2]
    return d


def unpack(d, wrap=lambda a: a):
    """The arrays of inputs() -> (outputs six-tuple, data dict) as train.py names them."""
    g = lambda key: wrap(d[key]) if key in d else None
    outputs = ([g(f"pred_disp{k}") for k in range(3)], [g(f"pred_conf{k}") for k in range(3)],
               [g(f"disp0_{k}") for k in range(3)], [g(f"disp1_{k}") for k in range(3)],
               [g(f"conf0_{k}") for k in range(3)], [g(f"conf1_{k}") for k in range(3)])
    data = {k: wrap(d[k]) for k in ("gt", "validgt", "im2_mono", "gt_right", "validgt_right", "im3_mono")}
    return outputs, data


def reference_loss(ut, outputs, data, args, log):
    """train.py:281-379, evaluated with the reference's three functions; ``log`` collects the terms."""
    normalize, estimate_normals, correlation_score = ut.normalize, ut.estimate_normals, ut.correlation_score
    pred_disps, pred_confs, disps0, disps1, confs0, confs1 = outputs
    Wd = data["gt"].shape[-1]
    xx = torch.arange(Wd).reshape(1, 1, 1, Wd).float()
    mask = (data["validgt"] > 0) & (data["gt"] < args["maxdisp"])
    th = args["lrc_th"]
    div = math.log(1 + math.exp(th))
    gain = Wd / args["normal_gain"]
    n2 = estimate_normals(data["im2_mono"], normal_gain=gain)
    n3 = estimate_normals(data["im3_mono"], normal_gain=gain)
    losses = []

    def keep(name, w, value, always=False):
        log[name] = value.detach()
        if always or not torch.isnan(value):
            losses.append(w * value)

    def bce(disp, conf, m, gt):
        e = (disp[m] - gt[m]).abs()
        tgt = F.softplus(th - e).detach().float() / div
        ok = torch.logical_not(torch.isnan(tgt)) & torch.logical_not(torch.isnan(conf[m]))
        return F.binary_cross_entropy(torch.clip(conf[m][ok], 0, 1), torch.clip(tgt[ok], 0, 1))

    n = len(pred_disps)
    for i in range(n):
        w = (0.9 ** (15 / (n - 1))) ** (n - i - 1)
        keep(f"seq_l1_{i}", w, (pred_disps[i][mask] - -data["gt"][mask]).abs().mean(), always=True)
        if args["use_normal_loss"]:
            na = estimate_normals(normalize(-pred_disps[i])[0], normal_gain=gain)
            keep(f"seq_n_{i}", w * 10, (1 - correlation_score(na, n2))[mask].mean())
        if pred_confs[i] is not None:
            keep(f"seq_bce_{i}", w, bce(pred_disps[i], pred_confs[i], mask, data["gt"]))
    w = 1.0   # the stale i_weight of the last prediction

    def coarse(tag, disps, confs, gt, m, bm, normals_mono, drop_bce):
        for i, (d, c) in enumerate(zip(disps, confs)):
            if d is None or torch.isnan(d).any():
                continue
            if i == 2:
                tmp = (d[m] - gt[m]).abs()
            else:
                tmp = (d[m & bm] - gt[m & bm]).abs()
                if args["use_normal_loss_on_coarse"]:
                    na = estimate_normals(normalize(d)[0], normal_gain=gain)
                    keep(f"{tag}_n_{i}", w * 10, (1 - correlation_score(na, normals_mono))[m & bm].mean())
            keep(f"{tag}_l1_{i}", 1.0, tmp.mean())
            if c is not None:
                keep(f"{tag}_bce_{i}", 1.0, bce(d, c, m, gt), always=not drop_bce)

    lb = xx - data["gt"] >= 0 if args["use_border_mask"] else torch.ones_like(data["gt"]).bool()
    coarse("left", disps0, confs0, data["gt"], mask, lb, n2, False)
    if "gt_right" in data:
        mr = (data["validgt_right"] > 0) & (data["gt_right"] < args["maxdisp"])
        rb = xx + data["gt_right"] < Wd if args["use_border_mask"] else torch.ones_like(data["gt_right"]).bool()
        coarse("right", disps1, confs1, data["gt_right"], mr, rb, n3, True)
    return sum(losses)


def main():
    _, ut, _ = _load_reference()
    d = inputs()
    leaves = {}

    def wrap(a):
        t = torch.from_numpy(a.copy())
        return t

    outputs, data = unpack(d, wrap)
    for group in outputs:
        for t in group:
            if t is not None:
                t.requires_grad_(True)
    log = {}
    total = reference_loss(ut, outputs, data, ARGS, log)
    total.backward()
    out = {f"in_{k}": v for k, v in d.items()}
    out.update({f"term_{k}": v.numpy() for k, v in log.items()})
    out["total"] = total.detach().numpy()
    names = [[f"pred_disp{k}" for k in range(3)], [f"pred_conf{k}" for k in range(3)],
             [f"disp0_{k}" for k in range(3)], [f"disp1_{k}" for k in range(3)],
             [f"conf0_{k}" for k in range(3)], [f"conf1_{k}" for k in range(3)]]
    for group, ns in zip(outputs, names):
        for t, nm in zip(group, ns):
            if t is not None:
                out[f"grad_{nm}"] = t.grad.numpy()
    for k, v in ARGS.items():
        out[f"arg_{k}"] = np.asarray(v)
    path = os.path.join(HERE, "losses.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes; total", float(total), "terms", len(log))


if __name__ == "__main__":
    main()
