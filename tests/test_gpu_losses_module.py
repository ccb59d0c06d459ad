"""stereoanywhere_amd.losses (sequence_loss / coarse_loss / training_loss over the fused HIP loss)
against the reference-generated fixture tests/golden/losses.npz and against torch.autograd of the
float64 restatement (tests/losses_ref.py), under the bound of tests/test_gpu_losses.py: e_ref =
max |fp32 torch - fp64| on the CPU, asserted > 0, and max |hip - fp64| <= 4 e_ref; two runs, equal bits.

The chain.  Nine maps come from a 3 x 3 convolution of one image (nine shifted multiply-adds in
float64, written out in torch on either side, then rounded to fp32 with ``.float()``, the cast the
module asks of a caller whose activations are not fp32): the gradients of its 81 weights are compared
under the same bound.  The convolution is not code under test; in float64 its own rounding stays out of
the comparison, so what is measured is the loss and its adjoint.  The target normals of the chain are
``ops.mono_normals`` of the mono maps, handed to the restatement as fp32 data (the kernel is pinned to
the reference elsewhere); the fixture test uses the restatement's own float64 normals."""
import os
import types

import numpy as np
import pytest
import torch

import losses_ref as ref
from stereoanywhere_amd import losses, ops

pytestmark = pytest.mark.gpu
dev = "cuda"
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "losses.npz")
STEMS = ("pred_disp", "pred_conf", "disp0_", "disp1_", "conf0_", "conf1_")


def g(a, grad=False):
    if a is None:
        return None
    t = torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(dev)
    return t.requires_grad_(True) if grad else t


def c(t):
    torch.cuda.synchronize()
    return t.detach().cpu().numpy()


def bound(label, got, want64, want32):
    got, want64, want32 = (np.asarray(a, dtype=np.float64) for a in (got, want64, want32))
    e_ref = np.abs(want32 - want64).max()
    err = np.abs(got - want64).max()
    print(f"{label}: err {err:.3g}, e_ref {e_ref:.3g}, err/e_ref {err / e_ref if e_ref else float('inf'):.3g}")
    assert e_ref > 0, label + ": e_ref is 0"
    assert np.isfinite(got).all() and err <= 4 * e_ref, label


@pytest.fixture(scope="module")
def golden():
    z = np.load(GOLDEN)
    return {k: z[k] for k in z.files}


def unpack(golden):
    d = {k[3:]: v for k, v in golden.items() if k.startswith("in_")}
    outputs = tuple([d.get(f"{stem}{k}") for k in range(3)] for stem in STEMS)
    data = {k: d[k] for k in ("gt", "validgt", "im2_mono", "gt_right", "validgt_right", "im3_mono")}
    args = {k[4:]: v.item() for k, v in golden.items() if k.startswith("arg_")}
    return outputs, data, args


def to_gpu(outputs, data, grad=True):
    return tuple([g(a, grad) for a in group] for group in outputs), {k: g(v) for k, v in data.items()}


def leaves(outputs):
    """(maps, confidences) in the order of losses_ref.training_loss_and_grads, with the fixture's names."""
    maps = [(f"{STEMS[i]}{k}", outputs[i][k]) for i in (0, 2, 3) for k in range(3) if outputs[i][k] is not None]
    confs = [(f"{STEMS[i]}{k}", outputs[i][k]) for i in (1, 4, 5) for k in range(3) if outputs[i][k] is not None]
    return maps, confs


def test_training_loss_on_the_fixture(golden):
    """The reference-generated total, terms and gradients are the fp32 side of the bound."""
    outputs, data, args = unpack(golden)
    t64, terms64, gm64, gc64 = ref.training_loss_and_grads(outputs, data, args, torch.float64)
    runs = []
    for _ in range(2):
        go, gd = to_gpu(outputs, data)
        total, terms = losses.training_loss(go, gd, types.SimpleNamespace(**args))
        total.backward()
        runs.append((total, terms, go))
    (total, terms, go), (total2, terms2, go2) = runs
    assert total.dtype == torch.float32 and total.dim() == 0
    assert torch.equal(total, total2) and all(torch.equal(terms[k], terms2[k]) for k in terms)
    bound("fixture total", c(total), t64, golden["total"])
    assert torch.equal(terms["total"], total.detach())
    for block, tag, want in zip(("sequence", "left", "right"), ("seq", "left", "right"), terms64):
        got = c(terms[block])
        assert got.shape == want.shape
        for k in range(want.shape[0]):
            for j, t in enumerate(("l1", "n", "bce")):
                key = f"term_{tag}_{t}_{k}"
                if key in golden:
                    bound(key, got[k, j], want[k, j], golden[key])
                else:
                    assert got[k, j] == 0 and want[k, j] == 0, key
    (mnames, cnames), (_, _) = leaves(go), leaves(go2)
    for (name, t), (_, t2), w64 in zip(mnames + cnames, sum(leaves(go2), []), gm64 + gc64):
        assert torch.equal(t.grad, t2.grad), name + ": two runs differ"
        bound(f"grad_{name}", c(t.grad), w64, golden[f"grad_{name}"])


# ------------------------------------------------------------------------------------ the chain
def conv9(img, w):
    """[B,1,H,W] image, [9,3,3] weights -> nine [B,1,H,W] maps: zero-padded 3 x 3 cross-correlation."""
    H, W = img.shape[-2:]
    p = torch.nn.functional.pad(img, [1, 1, 1, 1])
    out = []
    for k in range(w.shape[0]):
        acc = 0
        for dy in range(3):
            for dx in range(3):
                acc = acc + w[k, dy, dx] * p[:, :, dy:dy + H, dx:dx + W]
        out.append(acc)
    return out


def chain_problem():
    """An image, weights that make map k about gt (left) / gt_right plus a smooth offset of at least
    0.05, confidences, mono maps."""
    # no constant plane here: its normals term divides by mx - mn + 1e-4, and a convolution's fp32 rounding
    # of a constant plane is amplified 1e4 times in the fp32 side of the bound, which then says nothing
    left = ref.make_case(2, 9, 33, 6, seed=31, constant_plane=False)
    right = ref.make_case(2, 9, 33, 3, seed=32, constant_plane=False)
    rng = np.random.default_rng(5)
    w = rng.uniform(-0.2, 0.2, (9, 3, 3))
    img = rng.uniform(0.5, 1.5, left["gt"].shape)
    data = dict(gt=left["gt"], validgt=left["valid"], im2_mono=left["mono"], gt_right=right["gt"],
                validgt_right=right["valid"], im3_mono=right["mono"])
    # biases (data, no gradient): the fixture-like maps minus the conv of the image, so that the chain's
    # maps are those maps exactly up to rounding and keep their distance from the kinks
    want = [-left["signs"][k] * left["maps"][k] for k in range(3)] + \
           [left["signs"][3 + k] * left["maps"][3 + k] for k in range(3)] + \
           [right["signs"][k] * right["maps"][k] for k in range(3)]
    conv = conv9(torch.from_numpy(img), torch.from_numpy(w))
    bias = [torch.from_numpy(m.astype(np.float64)) - cv for m, cv in zip(want, conv)]
    confs = dict(pred=[None, None, left["confs"][2]], c0=[left["confs"][3], left["confs"][4], None],
                 c1=[right["confs"][0], None, right["confs"][2]])
    args = dict(maxdisp=left["maxdisp"], lrc_th=1.0, normal_gain=10, use_normal_loss=True,
                use_normal_loss_on_coarse=True, use_border_mask=True)
    return img, w, bias, confs, data, args


def chain_reference(dtype, which, targets):
    img, w, bias, confs, data, args = chain_problem()
    wt = torch.from_numpy(w).to(dtype).requires_grad_(True)
    maps = [m + b.to(dtype) for m, b in zip(conv9(torch.from_numpy(img).to(dtype), wt), bias)]
    cf = {k: [None if a is None else torch.from_numpy(a).to(dtype) for a in v] for k, v in confs.items()}
    d = {k: torch.from_numpy(v).to(dtype) for k, v in data.items()}
    tl, tr = (torch.from_numpy(t).to(dtype) for t in targets)
    gain = d["gt"].shape[-1] / args["normal_gain"]
    kw = dict(maxdisp=args["maxdisp"], gain=gain, lrc_th=1.0)
    total = 0
    if which in ("sequence", "training"):
        total = total + ref.loss_terms(ref.sequence_maps(maps[:3], use_normal_loss=True, pred_confs=cf["pred"]),
                                       d["gt"], d["validgt"], target=tl, border="none", **kw)[0]
    if which in ("coarse", "training"):
        total = total + ref.loss_terms(ref.coarse_maps(maps[3:6], cf["c0"], side="left",
                                                       use_normal_loss_on_coarse=True),
                                       d["gt"], d["validgt"], target=tl, border="left", **kw)[0]
    if which == "training":
        total = total + ref.loss_terms(ref.coarse_maps(maps[6:], cf["c1"], side="right",
                                                       use_normal_loss_on_coarse=True),
                                       d["gt_right"], d["validgt_right"], target=tr, border="right", **kw)[0]
    total.backward()
    return float(total.detach()), wt.grad.double().numpy()


def chain_hip(which):
    img, w, bias, confs, data, args = chain_problem()
    wt = torch.from_numpy(w).to(dev).requires_grad_(True)
    maps = [(m + b.to(dev)).float() for m, b in zip(conv9(torch.from_numpy(img).to(dev), wt), bias)]
    cf = {k: [g(a) for a in v] for k, v in confs.items()}
    d = {k: g(v) for k, v in data.items()}
    kw = dict(maxdisp=args["maxdisp"], normal_gain=10, lrc_th=1.0)
    if which == "sequence":
        total = losses.sequence_loss(maps[:3], d["gt"], d["validgt"], mono=d["im2_mono"], use_normal_loss=True,
                                     pred_confs=cf["pred"], **kw)
    elif which == "coarse":
        total = losses.coarse_loss(maps[3:6], cf["c0"], d["gt"], d["validgt"], side="left", mono=d["im2_mono"],
                                   use_normal_loss_on_coarse=True, use_border_mask=True, **kw)
    else:
        total, _ = losses.training_loss((maps[:3], cf["pred"], maps[3:6], maps[6:], cf["c0"], cf["c1"]), d, args)
    total.backward()
    return total, wt.grad


@pytest.mark.parametrize("which", ["sequence", "coarse", "training"])
def test_chain_parameter_gradients(which):
    d = chain_problem()[4]
    targets = [c(ops.mono_normals(g(d[k]), 33 / 10)) for k in ("im2_mono", "im3_mono")]
    t64, g64 = chain_reference(torch.float64, which, targets)
    t32, g32 = chain_reference(torch.float32, which, targets)
    (total, grad), (total2, grad2) = chain_hip(which), chain_hip(which)
    assert total.dtype == torch.float32 and torch.equal(total, total2) and torch.equal(grad, grad2)
    bound(f"{which} total", c(total), t64, t32)
    bound(f"{which} grad_weights", c(grad), g64, g32)
    used = {"sequence": slice(0, 3), "coarse": slice(3, 6), "training": slice(0, 9)}[which]
    assert np.abs(c(grad)[used]).min() > 0 and (which == "training" or not np.delete(c(grad), np.r_[used], 0).any())


# ------------------------------------------------------------------------- the Python layer
def small(grad):
    case = ref.make_case(2, 5, 7, 3, seed=9)
    preds = [g(-s * m, grad) for m, s in zip(case["maps"], case["signs"])]
    confs = [g(a, grad) for a in case["confs"]]
    return case, preds, confs, g(case["gt"]), g(case["valid"]), g(case["mono"])


def test_grad_mode_off_is_the_plain_forward():
    case, preds, confs, gt, valid, mono = small(True)
    kw = dict(maxdisp=case["maxdisp"], mono=mono, use_normal_loss=True, pred_confs=confs)
    with_grad = losses.sequence_loss(preds, gt, valid, **kw)
    assert with_grad.grad_fn is not None
    with torch.no_grad():
        off = losses.sequence_loss(preds, gt, valid, **kw)
    assert off.grad_fn is None and not off.requires_grad and torch.equal(off, with_grad.detach())
    plain = losses.sequence_loss([p.detach() for p in preds], gt, valid, **dict(kw, pred_confs=[x.detach() for x in confs]))
    assert plain.grad_fn is None and torch.equal(plain, off)


def test_saved_for_backward_is_the_inputs_and_the_record():
    case, preds, confs, gt, valid, mono = small(True)
    total, terms = losses.loss_terms([ops.LossMap(p, cf, -1, 0, 1.0, 0.5, 0.25) for p, cf in zip(preds, confs)], gt,
                                     valid, maxdisp=case["maxdisp"], target=ops.mono_normals(mono, 0.7), gain=0.7)
    fn = total.grad_fn
    while fn is not None and "LossTermsFn" not in type(fn).__name__:
        fn = fn.next_functions[0][0]
    assert fn is not None
    inputs = {t.data_ptr() for t in preds + confs + [gt, valid]}
    small_ones = []
    for t in fn.saved_tensors:
        if t is None or t.data_ptr() in inputs or tuple(t.shape) == (2, 3, 5, 7):   # (the target normals: an input)
            continue
        small_ones.append(t)
    assert len(small_ones) == 1 and small_ones[0].dtype == torch.float64
    assert small_ones[0].numel() == 4 + 8 * 3 + 2 * 3 * 2   # the record: a few doubles per map
    assert terms.shape == (3, 3) and not terms.requires_grad


def test_refusals():
    case, preds, confs, gt, valid, mono = small(False)
    kw = dict(maxdisp=case["maxdisp"])
    with pytest.raises(ValueError, match="at least 2 predictions"):
        losses.sequence_loss(preds[:1], gt, valid, **kw)
    with pytest.raises(RuntimeError, match="must be on the GPU"):
        losses.sequence_loss([p.cpu() for p in preds], gt, valid, **kw)
    with pytest.raises(RuntimeError, match="gt must be on the GPU"):
        losses.sequence_loss(preds, gt.cpu(), valid, **kw)
    with pytest.raises(RuntimeError, match="must be float32"):
        losses.sequence_loss([p.half() for p in preds], gt, valid, **kw)
    with pytest.raises(RuntimeError, match="must be float32"):
        losses.sequence_loss(preds, gt, valid.bool(), **kw)
    with pytest.raises(RuntimeError, match="with gt's B, H, W"):
        losses.sequence_loss([p[:, :, :, :5] for p in preds], gt, valid, **kw)
    with pytest.raises(RuntimeError, match=r"must be \[B,1,H,W\]"):
        losses.sequence_loss([p[:, 0] for p in preds], gt, valid, **kw)
    with pytest.raises(ValueError, match="needs the mono map"):
        losses.sequence_loss(preds, gt, valid, use_normal_loss=True, **kw)
    with pytest.raises(ValueError, match="side must be 'left' or 'right'"):
        losses.coarse_loss(preds, confs, gt, valid, side="top", **kw)
    with pytest.raises(ValueError, match="three disparities and three confidences"):
        losses.coarse_loss(preds[:2], confs[:2], gt, valid, side="left", **kw)
    with pytest.raises(ValueError, match="args has no maxdisp"):
        losses.training_loss((preds, [None] * 3, preds, preds, confs, confs),
                             dict(gt=gt, validgt=valid, im2_mono=mono, im3_mono=mono), {})
    none = losses.coarse_loss([None] * 3, [None] * 3, gt, valid, side="left", **kw)
    assert float(none) == 0.0


def test_no_host_synchronisation_in_the_python_layer():
    """torch's sync debug mode raises on any synchronising torch call (.item(), nonzero, a boolean mask,
    a host copy).  It sees torch calls only: that the kernels' launches do not synchronise is by
    construction (no HIP call but the launches)."""
    case, preds, confs, gt, valid, mono = small(True)
    args = dict(maxdisp=case["maxdisp"], lrc_th=1.0, normal_gain=10, use_normal_loss=True,
                use_normal_loss_on_coarse=True, use_border_mask=True)
    data = dict(gt=gt, validgt=valid, im2_mono=mono, im3_mono=mono, gt_right=gt, validgt_right=valid)
    coarse = [p.detach().neg().requires_grad_(True) for p in preds]
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        total, terms = losses.training_loss((preds, [None, None, confs[2]], coarse, coarse, confs, [confs[0], None, None]),
                                            data, args)
        total.backward()
        seq = losses.sequence_loss(preds, gt, valid, maxdisp=case["maxdisp"])
        left = losses.coarse_loss(coarse, confs, gt, valid, maxdisp=case["maxdisp"], side="left")
        (seq + left).backward()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert np.isfinite(c(total)) and all(np.isfinite(c(p.grad)).all() for p in preds + coarse + confs)
