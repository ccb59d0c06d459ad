"""Generate tests/golden/insitu_*.npz: the REFERENCE's own training forward and backward, captured on the
CPU at every boundary where this package has a differentiable drop-in ("In situ").

Test infrastructure only, run where the reference is mounted (see make_golden.py):

    python tests/golden/make_golden_insitu.py

The run: StereoAnywhere(volume_corruption_prob=0), seeded weights (seed 0), train mode with freeze_bn()
(train.py:245), every parameter trainable, forward(test_mode=False) with 4 iterations on
synth.synthetic_batch(2, 64, 128, 24.0, seed0=1) in float32 under grad mode, the loss of train.py:281-379 as
tests/losses_ref.py restates it (ground truth: the synthetic pair's disparity, for both views), backward().

The capture: the names of FUNCTIONS in the reference module's namespace, CorrBlock1D's three methods and the
mono hourglass's forward are wrapped with recorders.  A recorder
hands each floating input to the original function through an identity view (so that the gradient that
leaves *this call* for the input is kept apart from the other consumers' gradients), or, when the input has
no graph upstream, as a fresh leaf that requires grad (the same values); it hooks every output for the
gradient that arrives there.  Only data is written: float32 arrays and JSON lists of names and shapes.

Files: no committed file may exceed MAX_BYTES (1 MiB), which the run's dense float32 volumes do many times over,
so the arrays are spread, in key order, over insitu_NN.npz (S1, S3-S8 and the head) and insitu_hourglass_NN.npz
(S2), each below the limit; byte-identical arrays are stored once.  insitu.json holds the run's settings, every
array's shape, the aliases and which file holds which key; tests/insitu_util.py merges them back into one
dictionary.  Every site keeps B = 2.  A second run with peaked classifier volumes adds s3p.* (PEAK_GAIN below).
"""
from __future__ import annotations

import json
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from make_golden import REF_ARGS, _load_reference, _single_thread_lsq  # noqa: E402
import losses_ref  # noqa: E402
import lsq_lrc_ref  # noqa: E402
from stereoanywhere_amd import synth  # noqa: E402

ITERS = 4
B, H, W, D, SEED = 2, 64, 128, 24.0, 1
LOSS_ARGS = dict(maxdisp=20.0, lrc_th=1.0, normal_gain=10, use_normal_loss=True, use_normal_loss_on_coarse=True,
                 use_border_mask=True)
MAX_BYTES = 1 << 20   # per file
# The seeded classifiers give nearly flat volumes (confidences below 0.02).  A second run with both classifiers'
# weights multiplied by PEAK_GAIN gives what a trained model gives, one sharp softmax peak per line and confidences up
# to 1; only its four estimate_* calls are kept, as s3p.*.
PEAK_GAIN = 64.0
FUNCTIONS = ("estimate_left_disparity", "estimate_right_disparity", "estimate_left_confidence",
             "estimate_right_confidence", "softlrc", "fuzzy_and", "weighted_lsq", "truncate_corr_volume_v2",
             "convex_upflow")


def _np(t):
    return t.detach().cpu().float().numpy().copy()


class Recorder:
    """calls[name]: a list of dicts(ins, kw, outs, gouts) in call order."""

    def __init__(self):
        self.calls = {}

    def feed(self, x):
        if not (torch.is_tensor(x) and x.is_floating_point()):
            return x
        if x.requires_grad:
            y = x.view_as(x)
            y.retain_grad()
            return y
        return x.detach().clone().requires_grad_(True)

    def watch(self, call, outs):
        call["outs"], call["gouts"] = list(outs), [None] * len(outs)
        for j, o in enumerate(outs):
            if torch.is_tensor(o) and o.requires_grad:
                o.register_hook(lambda g, j=j: call["gouts"].__setitem__(j, g.detach().clone()))

    def wrap(self, name, fn):
        def w(*a, **k):
            a = [self.feed(x) for x in a]
            out = fn(*a, **k)
            call = dict(ins=a, kw=k)
            self.watch(call, out if isinstance(out, (tuple, list)) else (out,))
            self.calls.setdefault(name, []).append(call)
            return out
        return w


def run(sa_mod, corr_mod, classifier_gain=1.0):
    pair = synth.synthetic_batch(B, H, W, D, seed0=SEED)
    torch.manual_seed(0)
    model = sa_mod.StereoAnywhere(dict(REF_ARGS, volume_corruption_prob=0))
    synth.load_seeded_weights(model, seed=0)
    with torch.no_grad():
        model.classifier_mono.weight.mul_(classifier_gain)
        model.classifier_monoconf.weight.mul_(classifier_gain)
    model.train()
    model.freeze_bn()
    rec = Recorder()
    saved = {n: getattr(sa_mod, n) for n in FUNCTIONS}
    for n in FUNCTIONS:
        setattr(sa_mod, n, rec.wrap(n, saved[n]))
    orig_corr, orig_init, orig_call = corr_mod.CorrBlock1D.corr, corr_mod.CorrBlock1D.__init__, corr_mod.CorrBlock1D.__call__
    corr_mod.CorrBlock1D.corr = staticmethod(rec.wrap("corr", orig_corr))
    blocks = []

    def init_w(self, fullcorr, *a, **k):
        fullcorr.retain_grad()                      # the total over every lookup of this block
        orig_init(self, fullcorr, *a, **k)
        blocks.append(dict(block=self, fullcorr=fullcorr, lookups=[]))

    def call_w(self, coords):
        assert not coords.requires_grad             # stereoanywhere.py:268
        out = orig_call(self, coords)
        call = dict(ins=[coords.detach().clone()], kw={})
        rec.watch(call, (out,))
        next(b for b in blocks if b["block"] is self)["lookups"].append(call)
        return out

    corr_mod.CorrBlock1D.__init__, corr_mod.CorrBlock1D.__call__ = init_w, call_w
    hg = model.hourglass_mono
    hg_forward = hg.forward

    def hourglass_w(x, features_left, features_right):
        x, fl, fr = rec.feed(x), [rec.feed(f) for f in features_left], [rec.feed(f) for f in features_right]
        out = hg_forward(x, features_left=fl, features_right=fr)
        call = dict(ins=[x] + fl + fr, kw={})
        rec.watch(call, (out,))
        rec.calls.setdefault("hourglass_mono", []).append(call)
        return out

    hg.forward = hourglass_w
    heads = {}

    def keep_head(name):
        def hook(_m, _i, o):
            o.retain_grad()                         # the total over every consumer of the volume
            heads[name] = o
        return hook

    hooks = [getattr(model, n).register_forward_hook(keep_head(n)) for n in ("classifier_mono", "classifier_monoconf")]
    try:
        # copies in torch's own 64-byte-aligned memory, not numpy's buffers, whose alignment changes from run to run
        t = {k: torch.from_numpy(pair[k]).clone() for k in ("left", "right", "mono_left", "mono_right")}
        outputs = model(t["left"], t["right"], t["mono_left"], t["mono_right"], iters=ITERS, test_mode=False)
    finally:
        for n in FUNCTIONS:
            setattr(sa_mod, n, saved[n])
        corr_mod.CorrBlock1D.corr = staticmethod(orig_corr)
        corr_mod.CorrBlock1D.__init__, corr_mod.CorrBlock1D.__call__ = orig_init, orig_call
        for h in hooks:
            h.remove()
        del hg.forward
    flows, _, c2, c3, l2, l3 = outputs
    returned = {"dispmono2": c2[1], "scaled_mde2": c2[2], "dispmono3": c3[1], "scaled_mde3": c3[2],
                "ldispmonoconf2": l2[1], "ldispmonoconf3": l3[1]}
    for v in returned.values():
        v.retain_grad()
    gt = torch.from_numpy(pair["disp"])[:, None].clone()
    data = dict(gt=gt, validgt=torch.ones_like(gt), im2_mono=t["mono_left"], gt_right=gt.clone(),
                validgt_right=torch.ones_like(gt), im3_mono=t["mono_right"])
    total = 0.0
    for maps, kw in losses_ref.training_calls(outputs, data, LOSS_ARGS):
        g, v = data[kw.pop("gt")], data[kw.pop("valid")]
        target = losses_ref.estimate_normals(data[kw.pop("target")[1]], kw["gain"])
        total = total + losses_ref.loss_terms(maps, g, v, kw["maxdisp"], target, kw["gain"], kw["border"], kw["lrc_th"])[0]
    total.backward()
    return dict(pair=pair, model=model, rec=rec, blocks=blocks, heads=heads, returned=returned, flows=flows,
                loss=float(total.detach()))


def collect(r):
    """The captured tensors as float32 arrays under site names, plus the metadata."""
    out, calls = {}, r["rec"].calls

    def put(prefix, call, in_names, out_names):
        for n, x in zip(in_names, call["ins"]):
            if n is None or not torch.is_tensor(x):
                continue
            out[f"{prefix}.{n}"] = _np(x)
            if x.grad is not None:
                out[f"{prefix}.g_{n}"] = _np(x.grad)
        for n, o, g in zip(out_names, call["outs"], call["gouts"]):
            out[f"{prefix}.{n}"] = _np(o)
            if g is not None:
                out[f"{prefix}.g_{n}"] = _np(g)

    assert len(calls["corr"]) == 2                          # the feature volume (:135), then the normals' (:136)
    put("s1", calls["corr"][0], ("f2", "f3"), ("out",))
    hg_call, = calls["hourglass_mono"]
    nf = (len(hg_call["ins"]) - 1) // 2
    put("s2", hg_call, ["x"] + [f"fl{i}" for i in range(nf)] + [f"fr{i}" for i in range(nf)], ("out",))
    dead = []
    for name, p in r["model"].hourglass_mono.named_parameters():
        if p.grad is None:
            dead.append(name)
        else:
            out[f"s2.p.{name}"] = _np(p.grad)
    for key, n in (("dL", "estimate_left_disparity"), ("dR", "estimate_right_disparity"),
                   ("cL", "estimate_left_confidence"), ("cR", "estimate_right_confidence")):
        assert len(calls[n]) == 1
        put(f"s3.{key}", calls[n][0], ("vol",), ("out",))
    assert len(calls["softlrc"]) == 2 and len(calls["fuzzy_and"]) == 2
    for i in range(2):
        put(f"s4.lrc{i}", calls["softlrc"][i], ("d2", "d3"), ("s2", "s3"))
        put(f"s4.and{i}", calls["fuzzy_and"][i], ("x", "y"), ("out",))
    put("s5", calls["weighted_lsq"][0], ("mde", "disp", "conf"), ("scale", "shift"))
    put("s6", calls["truncate_corr_volume_v2"][0], ("disp", "conf"), ("mask",))
    assert "s6.g_mask" not in out                           # detached at :203
    assert len(r["blocks"]) == 2
    for b, blk in enumerate(r["blocks"]):
        out[f"s7.{b}.fullcorr"] = _np(blk["fullcorr"])
        out[f"s7.{b}.g_fullcorr"] = _np(blk["fullcorr"].grad)
        assert len(blk["lookups"]) == ITERS
        for n, call in enumerate(blk["lookups"]):
            put(f"s7.{b}.{n}", call, ("coords",), ("taps",))
    assert len(calls["convex_upflow"]) == ITERS
    for n, call in enumerate(calls["convex_upflow"]):
        put(f"s8.{n}", call, ("flow", "mask"), ("up",))
    # the composed head: its inputs' total gradients, the mono maps, the returned entries
    out["head.g_vol_disp"] = _np(r["heads"]["classifier_mono"].grad)
    out["head.g_vol_conf"] = _np(r["heads"]["classifier_monoconf"].grad)
    out["head.mde2"], out["head.mde3"] = r["pair"]["mono_left"], r["pair"]["mono_right"]
    for k, v in r["returned"].items():
        out[f"head.{k}"], out[f"head.g_{k}"] = _np(v), _np(v.grad)
    for n, f in enumerate(r["flows"]):
        assert np.array_equal(_np(f), out[f"s8.{n}.up"])
    a = r["model"].args
    meta = dict(B=B, H=H, W=W, D=D, seed=SEED, iters=ITERS, loss=r["loss"], loss_args=LOSS_ARGS,
                lrc_th=a.lrc_th, mirror_attenuation=a.mirror_attenuation, mirror_conf_th=a.mirror_conf_th,
                corr_levels=a.corr_levels, corr_radius=a.corr_radius, n_downsample=a.n_downsample,
                inputs_sha256=synth.digest([r["pair"][k] for k in ("left", "right", "mono_left", "mono_right")]),
                hourglass_dead_parameters=dead,
                hourglass_weights_sha256=synth.digest([_np(v) for _, v in sorted(r["model"].hourglass_mono.state_dict().items())]),
                shapes={k: list(v.shape) for k, v in sorted(out.items())})
    return out, meta


def check(out):
    for k, v in out.items():
        assert np.isfinite(v).all(), f"{k} is not finite"
        if ".g_" in k or k.startswith("s2.p."):
            assert np.abs(v).max() > 0, f"{k} is all zero"
    # weighted_lsq: a non-empty band, no rank-deficient sample (the zero-gradient branches)
    m, d = (out[f"s5.{k}"].reshape(B, -1) for k in ("mde", "disp"))
    for b in range(B):
        keep = lsq_lrc_ref.band(torch.from_numpy(d[b]))[2].numpy()
        assert keep.sum() >= 2 and np.ptp(np.abs(m[b][keep])) > 0, f"weighted_lsq sample {b}: a zero-gradient branch"
        assert np.abs(out["s5.g_disp"].reshape(B, -1)[b]).max() > 0
    w2 = out["s7.0.fullcorr"].shape[-1]
    xs = np.concatenate([out[f"s7.0.{n}.coords"][:, 0].ravel() for n in range(ITERS)])
    assert ((xs < 0) | (xs >= w2)).any(), "no lookup coordinate outside [0, W2)"
    peak = out["s3.dL.vol"][:, 0].argmax(-1)
    assert ((peak == 0) | (peak == w2 - 1)).any(), "no soft-argmin line peaks at an end bin"
    print(f"lookup coordinates in [{xs.min():.2f}, {xs.max():.2f}], {int(((xs < 0) | (xs >= w2)).sum())} outside; "
          f"{int(((peak == 0) | (peak == w2 - 1)).sum())} soft-argmin lines peak at an end bin")


def peaked(r):
    """The four estimate_* calls of the PEAK_GAIN run under s3p.*."""
    out, calls = {}, r["rec"].calls
    for key, n in (("dL", "estimate_left_disparity"), ("dR", "estimate_right_disparity"),
                   ("cL", "estimate_left_confidence"), ("cR", "estimate_right_confidence")):
        call, = calls[n]
        out[f"s3p.{key}.vol"], out[f"s3p.{key}.g_vol"] = _np(call["ins"][0]), _np(call["ins"][0].grad)
        out[f"s3p.{key}.out"], out[f"s3p.{key}.g_out"] = _np(call["outs"][0]), _np(call["gouts"][0])
    for v in out.values():
        assert np.isfinite(v).all()
    p = torch.softmax(torch.from_numpy(out["s3p.dL.vol"][:, 0]), -1).amax(-1)
    conf = max(out["s3p.cL.out"].max(), out["s3p.cR.out"].max())
    print(f"peaked run: median / max line peak of the disparity softmax {float(p.median()):.3f} / {float(p.max()):.3f}, "
          f"largest confidence {conf:.3f}")
    assert float(p.median()) > 0.5 and conf > 0.9, "the peaked run is not peaked"
    assert all(np.abs(v).max() > 0 for k, v in out.items() if ".g_" in k)
    return out


def dedupe(out):
    """(kept arrays, {dropped key: the kept key with the same bytes})."""
    seen, kept, alias = {}, {}, {}
    for k in sorted(out):
        v = out[k]
        h = (v.shape, synth.digest([v]))
        if h in seen and v.nbytes > 64:
            alias[k] = seen[h]
        else:
            seen.setdefault(h, k)
            kept[k] = v
    return kept, alias


def shards(kept):
    """{file name: [keys]}: the keys in sorted order, the hourglass's (s2) apart from the rest, a new file
    whenever the next array would take the file past its size limit (sizes: zlib at the level the zip uses)."""
    files = {}
    for group, stem in ((False, "insitu"), (True, "insitu_hourglass")):
        n, room = -1, 0
        for k in sorted(kept):
            if k.startswith("s2.") != group:
                continue
            size = len(zlib.compress(kept[k].tobytes(), 6)) + 2 * len(k) + 256
            if size > room:
                n, room = n + 1, MAX_BYTES - 4096
            files.setdefault(f"{stem}_{n:02d}.npz", []).append(k)
            room -= size
    return files


def main():
    torch.set_num_threads(1)    # one summation order, whatever the machine
    sa_mod, _, corr_mod = _load_reference()
    restore = _single_thread_lsq(sa_mod)
    try:
        out, meta = collect(run(sa_mod, corr_mod))
    finally:
        restore()
    check(out)
    restore = _single_thread_lsq(sa_mod)
    try:
        out.update(peaked(run(sa_mod, corr_mod, PEAK_GAIN)))
    finally:
        restore()
    meta["peak_gain"] = PEAK_GAIN
    meta["shapes"] = {k: list(v.shape) for k, v in sorted(out.items())}
    out = {k: np.ascontiguousarray(v, np.float32) for k, v in out.items()}
    # About one run in ten differs from the others in the last place (the loss included; the cause was not found:
    # one thread and aligned inputs made it rarer, not impossible).  The committed index records the arrays' digest,
    # and a run that does not reproduce it writes nothing unless it is told to.
    meta["digest"] = synth.digest([out[k] for k in sorted(out)])
    index = os.path.join(HERE, "insitu.json")
    if os.path.exists(index) and "--accept" not in sys.argv:
        with open(index) as f:
            committed = json.load(f).get("digest")
        if committed is not None and committed != meta["digest"]:
            raise SystemExit(f"digest {meta['digest']} is not the committed {committed}: nothing written; run again, "
                             "or pass --accept if the capture was changed on purpose")
    kept, meta["aliases"] = dedupe(out)
    files = shards(kept)
    for old in sorted(os.listdir(HERE)):
        if old.startswith("insitu_") and old.endswith(".npz") and old not in files:
            raise SystemExit(f"stale fixture {old}: remove it")
    meta["files"] = files
    for name, keys in sorted(files.items()):
        path = os.path.join(HERE, name)
        np.savez_compressed(path, **{k: kept[k] for k in keys})
        print(name, os.path.getsize(path), "bytes", len(keys), "arrays")
        assert os.path.getsize(path) <= MAX_BYTES, name
    with open(os.path.join(HERE, "insitu.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    print("loss", meta["loss"], "digest", synth.digest([out[k] for k in sorted(out)]))


if __name__ == "__main__":
    main()
