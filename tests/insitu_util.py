"""The in-situ fixtures (tests/golden/make_golden_insitu.py: the reference's own training forward and backward
captured at every drop-in boundary) and the project's restatements run on them, site by site and as the
composed volume head.  Shared by tests/test_insitu_ref_cpu.py (the restatements are the reference's) and
tests/test_gpu_insitu.py (the HIP drop-ins are the restatements').

Every ``site_*`` function takes the merged fixture dictionary and a torch dtype and returns
{name: float64 numpy array} under the fixture's own key names, so that a caller compares key by key."""
from __future__ import annotations

import functools
import json
import os

import numpy as np
import torch
import torch.nn.functional as F

import corr_autograd_ref as corr_ref
import diffops_ref
import lsq_lrc_ref
import volume_stage_ref
from fixtures_util import GOLDEN

U = 2.0 ** -24


@functools.lru_cache(maxsize=1)
def load():
    """(arrays, meta): every file of the fixture merged, aliases resolved; arrays are read-only."""
    with open(os.path.join(GOLDEN, "insitu.json")) as f:
        meta = json.load(f)
    fix = {}
    for name, keys in meta["files"].items():
        z = np.load(os.path.join(GOLDEN, name), allow_pickle=False)
        assert sorted(z.files) == sorted(keys), name
        for k in z.files:
            fix[k] = z[k]
    for k, kept in meta["aliases"].items():
        fix[k] = fix[kept]
    assert sorted(fix) == sorted(meta["shapes"])
    for v in fix.values():
        v.setflags(write=False)
    return fix, meta


def t(a, dtype=torch.float32, device="cpu"):
    return torch.from_numpy(np.array(a, np.float32)).to(device=device, dtype=dtype)


def n64(x):
    return x.detach().double().cpu().numpy()


def e_ref(fix, ref64, key):
    """max |the reference's captured float32 value - the float64 restatement|."""
    return float(np.abs(fix[key].astype(np.float64) - ref64[key]).max())


def _backward(outs, grads, dtype):
    pairs = [(o, t(g, dtype)) for o, g in zip(outs, grads) if g is not None]
    torch.autograd.backward([o for o, _ in pairs], [g for _, g in pairs])


# ----------------------------------------------------------------------------------- S1: corr
def site_s1(fix, dtype=torch.float64):
    """corr_autograd_ref's einsums (float64 numpy; dtype is ignored) and the sums of their absolute terms."""
    f2, f3, g = fix["s1.f2"], fix["s1.f3"], fix["s1.g_out"][:, :, :, 0]
    sqrt_c = float(torch.sqrt(torch.tensor(float(f2.shape[1]), dtype=torch.float32)))
    out = {"s1.out": corr_ref.volume_forward(f2, f3, sqrt_c)[:, :, :, None]}
    out["s1.g_f2"], out["s1.g_f3"] = corr_ref.volume_backward(g, f2, f3, sqrt_c)
    mag = {"s1.out": corr_ref.volume_forward(np.abs(f2), np.abs(f3), sqrt_c)[:, :, :, None]}
    mag["s1.g_f2"], mag["s1.g_f3"] = corr_ref.volume_backward(np.abs(g), np.abs(f2), np.abs(f3), sqrt_c)
    return out, mag


# ----------------------------------------------------------------------------------- S3: soft-argmin
S3 = (("dL", diffops_ref.left_disparity), ("dR", diffops_ref.right_disparity),
      ("cL", diffops_ref.left_confidence), ("cR", diffops_ref.right_confidence))


S3_RUNS = ("s3", "s3p")   # the run proper (nearly flat classifier volumes) and the peaked one (PEAK_GAIN)


def s3_captured_sums(fix, s="s3"):
    """What autograd accumulates at each volume: the two calls' gradients added in float32."""
    return {f"{s}.g_vol_disp": fix[f"{s}.dL.g_vol"] + fix[f"{s}.dR.g_vol"],
            f"{s}.g_vol_conf": fix[f"{s}.cL.g_vol"] + fix[f"{s}.cR.g_vol"]}


def site_s3(fix, dtype=torch.float64, s="s3"):
    vd, vc = t(fix[f"{s}.dL.vol"], dtype).requires_grad_(), t(fix[f"{s}.cL.vol"], dtype).requires_grad_()
    outs = [fn((vd if k[0] == "d" else vc)[:, 0])[:, None] for k, fn in S3]
    _backward(outs, [fix[f"{s}.{k}.g_out"] for k, _ in S3], dtype)
    res = {f"{s}.{k}.out": n64(o) for (k, _), o in zip(S3, outs)}
    res[f"{s}.g_vol_disp"], res[f"{s}.g_vol_conf"] = n64(vd.grad), n64(vc.grad)
    return res


# ----------------------------------------------------------------------------------- S4: softlrc, fuzzy_and
def site_s4(fix, meta, dtype=torch.float64):
    """softlrc at :186 from the gradients that arrive at its outputs; the same with the products of :188-189
    folded in (what softlrc_conf replaces) from the gradients at the products; softlrc at :199, forward only
    (its only consumer is detached)."""
    th = meta["lrc_th"]
    d2, d3 = (t(fix[f"s4.lrc0.{k}"], dtype).requires_grad_() for k in ("d2", "d3"))
    s2, s3 = lsq_lrc_ref.softlrc(d2, d3, th=th)
    _backward([s2, s3], [fix["s4.lrc0.g_s2"], fix["s4.lrc0.g_s3"]], dtype)
    res = {"s4.lrc0.s2": n64(s2), "s4.lrc0.s3": n64(s3), "s4.lrc0.g_d2": n64(d2.grad), "s4.lrc0.g_d3": n64(d3.grad)}
    d2, d3, c2, c3 = (t(fix[k], dtype).requires_grad_() for k in ("s4.lrc0.d2", "s4.lrc0.d3", "s4.and0.x", "s4.and1.x"))
    p2, p3 = lsq_lrc_ref.softlrc(d2, d3, c2, c3, th=th)
    _backward([p2, p3], [fix["s4.and0.g_out"], fix["s4.and1.g_out"]], dtype)
    res.update({"s4.and0.out": n64(p2), "s4.and1.out": n64(p3), "s4.and0.g_x": n64(c2.grad), "s4.and1.g_x": n64(c3.grad),
                "s4.fused.g_d2": n64(d2.grad), "s4.fused.g_d3": n64(d3.grad)})
    with torch.no_grad():
        q2, q3 = lsq_lrc_ref.softlrc(t(fix["s4.lrc1.d2"], dtype), t(fix["s4.lrc1.d3"], dtype), th=th)
    res.update({"s4.lrc1.s2": n64(q2), "s4.lrc1.s3": n64(q3)})
    return res


# ----------------------------------------------------------------------------------- S5: weighted_lsq
def site_s5(fix, dtype=torch.float64):
    B = fix["s5.mde"].shape[0]
    m, d, c = (t(fix[f"s5.{k}"], dtype).requires_grad_() for k in ("mde", "disp", "conf"))
    scale, shift = lsq_lrc_ref.weighted_lsq(m.reshape(B, -1), d.reshape(B, -1), c.reshape(B, -1), dtype)
    _backward([scale, shift], [fix["s5.g_scale"].reshape(B), fix["s5.g_shift"].reshape(B)], dtype)
    return {"s5.scale": n64(scale).reshape(B, 1, 1, 1), "s5.shift": n64(shift).reshape(B, 1, 1, 1),
            "s5.g_mde": n64(m.grad), "s5.g_disp": n64(d.grad), "s5.g_conf": n64(c.grad)}


# ----------------------------------------------------------------------------------- S6: truncation
def volume5(a):
    """[B,H,W1,1,W2] (the corr contract) -> [B,1,H,W1,W2]."""
    return np.ascontiguousarray(np.moveaxis(a, 3, 1))


def site_s6(fix, meta, dtype=torch.float64):
    """The mask of :203, the product of :254 and the volume's gradient (the mask is detached)."""
    vol = t(volume5(fix["s1.out"]), dtype).requires_grad_()
    mask = volume_stage_ref.trunc_factor(t(fix["s6.disp"]), t(fix["s6.conf"]), meta["mirror_attenuation"],
                                         vol.shape[-1], dtype)
    prod = volume_stage_ref.stage(vol, trunc=(t(fix["s6.disp"]), t(fix["s6.conf"]), meta["mirror_attenuation"]), dtype=dtype)
    prod.backward(t(volume5(fix["s7.0.g_fullcorr"]), dtype))
    return {"s6.mask": n64(mask), "s7.0.fullcorr": np.moveaxis(n64(prod), 1, 3), "s1.g_out": np.moveaxis(n64(vol.grad), 1, 3)}


# ----------------------------------------------------------------------------------- S7: the lookups
def lookup_matrices(fix, meta, b=0):
    """One float64 coefficient matrix per iteration, from the captured (detached) coordinates."""
    W2 = fix[f"s7.{b}.fullcorr"].shape[-1]
    return [corr_ref.lookup_matrix(fix[f"s7.{b}.{n}.coords"][:, :1], W2, meta["corr_levels"], meta["corr_radius"])
            for n in range(meta["iters"])]


def _taps(pixels, like):
    B, Q, H, W1 = like.shape
    return pixels.reshape(B, H, W1, Q).transpose(0, 3, 1, 2)


def site_s7(fix, meta, dtype=torch.float64):
    """corr_autograd_ref (float64 numpy; dtype is ignored): every iteration's taps of both blocks and the fold of
    the summed scatters at each fullcorr, with the sums of the absolute terms."""
    L = meta["corr_levels"]
    res, mag = {}, {}
    As = lookup_matrices(fix, meta)
    for b in range(2):
        full = fix[f"s7.{b}.fullcorr"]
        W2 = full.shape[-1]
        pyr, apyr = corr_ref.pyramid_forward(full.reshape(-1, W2), L), corr_ref.pyramid_forward(np.abs(full).reshape(-1, W2), L)
        gp, agp = 0.0, 0.0
        for n, A in enumerate(As):
            like = fix[f"s7.{b}.{n}.taps"]
            res[f"s7.{b}.{n}.taps"] = _taps(corr_ref.lookup_forward(A, pyr), like)
            mag[f"s7.{b}.{n}.taps"] = _taps(corr_ref.lookup_forward(A, apyr), like)
            gp = gp + corr_ref.lookup_backward(A, fix[f"s7.{b}.{n}.g_taps"])
            agp = agp + corr_ref.lookup_backward(A, np.abs(fix[f"s7.{b}.{n}.g_taps"]))
        res[f"s7.{b}.g_fullcorr"] = corr_ref.pyramid_backward(gp, W2, L).reshape(full.shape)
        mag[f"s7.{b}.g_fullcorr"] = corr_ref.pyramid_backward(agp, W2, L).reshape(full.shape)
    return res, mag


# ----------------------------------------------------------------------------------- S8: convex up-sampling
def site_s8(fix, meta, dtype=torch.float64):
    res = {}
    f = 2 ** meta["n_downsample"]
    for n in range(meta["iters"]):
        flow, mask = (t(fix[f"s8.{n}.{k}"], dtype).requires_grad_() for k in ("flow", "mask"))
        up = diffops_ref.convex_upflow(flow, mask, f)
        up.backward(t(fix[f"s8.{n}.g_up"], dtype))
        res.update({f"s8.{n}.up": n64(up), f"s8.{n}.g_flow": n64(flow.grad), f"s8.{n}.g_mask": n64(mask.grad)})
    return res


# ----------------------------------------------------------------------------------- S2: the hourglass
def hourglass_module(meta):
    """blocks.Hourglass with the weights the capture ran: the seeded ones under the model's names."""
    from stereoanywhere_amd import blocks, synth
    hg = blocks.Hourglass(8, 8)
    sd = hg.state_dict()
    vals = synth.seeded_state_dict({"hourglass_mono." + k: tuple(v.shape) for k, v in sd.items()}, 0)
    hg.load_state_dict({k: torch.from_numpy(vals["hourglass_mono." + k]) for k in sd}, strict=True)
    assert synth.digest([n64(v).astype(np.float32) for _, v in sorted(hg.state_dict().items())]) == meta["hourglass_weights_sha256"]
    return hg.train()


def hourglass_inputs(fix, dtype=torch.float32, device="cpu"):
    """x in the module's [B,C,W2,H,W1] layout and the two feature lists, all requiring grad."""
    x = t(fix["s2.x"], dtype, device).permute(0, 1, 4, 2, 3).contiguous().requires_grad_()
    fl = [t(fix[f"s2.fl{i}"], dtype, device).requires_grad_() for i in range(4)]
    fr = [t(fix[f"s2.fr{i}"], dtype, device).requires_grad_() for i in range(4)]
    return x, fl, fr


def run_hourglass(fix, hg, dtype=torch.float32, device="cpu", **kw):
    """Forward and backward of one route -> {fixture key: float64 array} (reference layout), dead entries None."""
    hg = hg.to(device=device, dtype=dtype)
    hg.zero_grad(set_to_none=True)
    x, fl, fr = hourglass_inputs(fix, dtype, device)
    out = hg(x, fl, fr, **kw).permute(0, 1, 3, 4, 2)
    out.backward(t(fix["s2.g_out"], dtype, device))
    res = {"s2.out": n64(out), "s2.g_x": n64(x.grad.permute(0, 1, 3, 4, 2))}
    for i in range(4):
        res[f"s2.g_fl{i}"] = None if fl[i].grad is None else n64(fl[i].grad)
        res[f"s2.g_fr{i}"] = None if fr[i].grad is None else n64(fr[i].grad)
    for name, p in hg.named_parameters():
        res[f"s2.p.{name}"] = None if p.grad is None else n64(p.grad)
    return res


def rel_metric(got, ref64):
    """max |got - ref64| / max |ref64| (the metric of tests/test_gpu_volume_close_autograd.py)."""
    return float(np.abs(np.asarray(got, np.float64) - ref64).max() / np.abs(ref64).max())


# ----------------------------------------------------------------------------------- the composed volume head
class RefOps:
    """The restatements under the drop-ins' names and signatures, in one dtype on the CPU."""

    def __init__(self, dtype):
        self.dtype = dtype

    def softargmin_conf(self, vd, vc):
        return tuple(fn((vd if k[0] == "d" else vc)[:, 0])[:, None] for k, fn in S3)

    def softlrc(self, d2, d3, lrc_th):
        return lsq_lrc_ref.softlrc(d2, d3, th=lrc_th)

    def softlrc_conf(self, d2, d3, c2, c3, lrc_th):
        return lsq_lrc_ref.softlrc(d2, d3, c2, c3, th=lrc_th)

    def weighted_lsq(self, mde, disp, conf):
        B = mde.shape[0]
        scale, shift = lsq_lrc_ref.weighted_lsq(mde.reshape(B, -1), disp.reshape(B, -1), conf.reshape(B, -1), self.dtype)
        return scale.reshape(B, 1, 1, 1), shift.reshape(B, 1, 1, 1)

    def volume_stage(self, stereo, mono, truncate):
        disp, conf, atten = truncate
        mask = volume_stage_ref.trunc_factor(disp.detach(), conf.detach(), atten, stereo.shape[-1], self.dtype)
        return stereo * mask.detach(), mono

    def corr_block(self, fullcorr, radius, num_levels):
        ops = self

        class Block:
            def __call__(self, coords):
                B, H, W1, _, W2 = fullcorr.shape
                A = torch.from_numpy(corr_ref.lookup_matrix(n64(coords[:, :1]), W2, num_levels, radius)).to(ops.dtype)
                levels = [fullcorr.reshape(-1, W2)]
                for _ in range(1, num_levels):
                    w = levels[-1].shape[1] // 2
                    levels.append(0.5 * (levels[-1][:, 0:2 * w:2] + levels[-1][:, 1:2 * w:2]))
                taps = torch.einsum("pqm,pm->pq", A, torch.cat(levels, 1))
                return taps.reshape(B, H, W1, -1).permute(0, 3, 1, 2)
        return Block()


def mirror_detector(stereo_disp, mono_disp, stereo_conf, mono_conf, conf_th, step_gain=20):
    """utils.py:255-269 written out: (stereo_conf and mono_conf and mono nearer than stereo) or (not stereo_conf
    and mono_conf), through a steep sigmoid."""
    a = stereo_conf * mono_conf * torch.sigmoid(step_gain * (mono_disp - stereo_disp))
    b = (1 - stereo_conf) * mono_conf
    return torch.sigmoid(step_gain * ((a + b - a * b) - conf_th))


HEAD_OUTPUTS = ("dispmono2", "dispmono3", "ldispmonoconf2", "ldispmonoconf3", "scaled_mde2", "scaled_mde3")


def head_inputs(fix, dtype=torch.float32, device="cpu"):
    """(vol_disp, vol_conf, stereo volume) [B,1,H,W1,W2] requiring grad, the mono maps, the coordinates."""
    vols = [t(a, dtype, device).requires_grad_() for a in (fix["s3.dL.vol"], fix["s3.cL.vol"], volume5(fix["s1.out"]))]
    mde = [t(fix[k], dtype, device) for k in ("head.mde2", "head.mde3")]
    return vols, mde


def head(ops, vols, mde, fix, meta, dtype=torch.float32, device="cpu"):
    """stereoanywhere.py:174-271 wired as INTEGRATION.md section 2 says, from ``ops`` (RefOps, or the drop-ins)
    and the torch glue between them -> {name: tensor}: the six returned coarse entries and every iteration's
    taps of both blocks."""
    vol_disp, vol_conf, stereo = vols
    mde2, mde3 = mde
    nd = 2 ** meta["n_downsample"]
    mde2_lr, mde3_lr = (F.interpolate(m, scale_factor=1 / nd, mode="bilinear", align_corners=True) for m in (mde2, mde3))
    up = lambda m: F.interpolate(m, scale_factor=nd, mode="bilinear", align_corners=True)
    dL, dR, cL, cR = ops.softargmin_conf(vol_disp, vol_conf)                                        # :174-177
    out = {"dispmono2": up(dL) * nd, "dispmono3": up(dR) * nd, "ldispmonoconf2": up(cL), "ldispmonoconf3": up(cR)}
    conf2, conf3 = ops.softlrc_conf(dL, dR, cL, cR, meta["lrc_th"])                                # :186-189
    scale, shift = ops.weighted_lsq(torch.cat([mde2_lr, mde3_lr], 1), torch.cat([dL, dR], 1), torch.cat([conf2, conf3], 1))
    smde2_lr = torch.sum(scale * mde2_lr + shift, dim=1, keepdim=True)                              # :194-197
    smde3_lr = torch.sum(scale * mde3_lr + shift, dim=1, keepdim=True)
    out["scaled_mde2"] = torch.sum(scale * mde2 + shift, dim=1, keepdim=True) * nd
    out["scaled_mde3"] = torch.sum(scale * mde3 + shift, dim=1, keepdim=True) * nd
    lrc_mde2, _ = ops.softlrc(smde2_lr, smde3_lr, meta["lrc_th"])                                   # :199
    mirror = mirror_detector(dL, smde2_lr, conf2, lrc_mde2, meta["mirror_conf_th"]).detach()        # :202 (detached at :203)
    stereo_full, mono_full = ops.volume_stage(stereo, vol_disp, (smde2_lr, mirror, meta["mirror_attenuation"]))
    blocks = [ops.corr_block(v.squeeze(1).unsqueeze(3), radius=meta["corr_radius"], num_levels=meta["corr_levels"])
              for v in (stereo_full, mono_full)]                                                   # :253-259
    for n in range(meta["iters"]):                                                                  # :268-271
        coords = t(fix[f"s7.0.{n}.coords"], dtype, device)
        for b, blk in enumerate(blocks):
            out[f"taps.{b}.{n}"] = blk(coords)
    out["mirror"], out["smde2_lr"] = mirror, smde2_lr.detach()
    return out


def head_backward(out, fix, meta, dtype=torch.float32, device="cpu"):
    """backward() from the captured gradients of exactly the head's outputs."""
    outs = [out[k] for k in HEAD_OUTPUTS]
    grads = [t(fix[f"head.g_{k}"], dtype, device) for k in HEAD_OUTPUTS]
    for b in range(2):
        for n in range(meta["iters"]):
            outs.append(out[f"taps.{b}.{n}"])
            grads.append(t(fix[f"s7.{b}.{n}.g_taps"], dtype, device))
    torch.autograd.backward(outs, grads)


HEAD_GRADS = ("head.g_vol_disp", "head.g_vol_conf", "head.g_stereo")


def head_captured(fix):
    return {"head.g_vol_disp": fix["head.g_vol_disp"], "head.g_vol_conf": fix["head.g_vol_conf"],
            "head.g_stereo": volume5(fix["s1.g_out"])}


def run_head(ops, fix, meta, dtype=torch.float32, device="cpu"):
    """-> ({output name: float64 array}, {HEAD_GRADS name: float64 array})."""
    vols, mde = head_inputs(fix, dtype, device)
    out = head(ops, vols, mde, fix, meta, dtype, device)
    head_backward(out, fix, meta, dtype, device)
    return {k: n64(v) for k, v in out.items()}, dict(zip(HEAD_GRADS, (n64(v.grad) for v in vols)))
