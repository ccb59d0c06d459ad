"""Shared by tests/test_gpu_large_offsets.py and tests/test_large_offsets_table_cpu.py: the list of `long`
stride parameters of include/stereoanywhere_hip.h (derived from the header, as _native.SIGNATURES is), the
table that says what covers each of them, and the far-stride harness.

A far-stride row calls one entry point with B = 2 on views of one arena per role (input, output) whose
batch stride is FAR = 2^31 + 64 floats: image 1 starts past 2^31 elements and past 2^33 bytes, so a batch
offset formed in 32 bits (elements or bytes) lands somewhere else.  The row runs with the far stride on one
parameter at a time, then on all of them together, and every output must equal, bit for bit, the same call
on dense tensors.  Only the two images of an arena are ever touched.

TABLE maps (owner, parameter) to one of
  ("far", row)            a row of FAR_ROWS below runs it on the GPU (owner: entry point or struct);
  ("gated", "file:line")  the entry point refuses the far value before any launch; GATED holds the call that
                          test_large_offsets_table_cpu.py makes to see the refusal.
"""
from __future__ import annotations

import ctypes
import re
from typing import Callable, Dict, List, Tuple

import torch

from stereoanywhere_amd import _native as N

FAR = (1 << 31) + 64          # floats between image 0 and image 1
SLOT = 1 << 22                # floats of one arena that an image's tensors may take (16 MiB)
_STRIDE_NAME = re.compile(r"(_bs|bstride|stride\w*|^disp_ts|^sb|^sh|^sj|^sk)$")


# ------------------------------------------------------------------------------- the header's parameters
def header_stride_params(text: str = None) -> List[Tuple[str, str]]:
    """(owner, name) of every `long` struct field and `long` prototype parameter of the header whose name is
    a stride's (*_bs, *_bstride, *stride*, disp_ts, sb / sh / sj / sk), in the header's order."""
    text = open(N.HEADER).read() if text is None else text
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    text = re.sub(r"^[ \t]*#.*$", " ", text, flags=re.M)
    found = []

    def struct(m):
        for line in m.group(1).split(";"):
            line = " ".join(line.split())
            if line.startswith("long "):
                found.extend((m.group(2), d.strip()) for d in line[5:].split(","))
        return " "
    text = re.sub(r"\btypedef\s+struct\s*\w*\s*\{([^{}]*)\}\s*(\w+)\s*;", struct, text)
    for m in re.finditer(r"\b(sa_\w+)\s*\(([^()]*)\)", text):
        for arg in m.group(2).split(","):
            parts = arg.split()
            if len(parts) == 2 and parts[0] == "long":
                found.append((m.group(1), parts[1]))
    return [(o, p) for o, p in found if _STRIDE_NAME.search(p)]


# ------------------------------------------------------------------------------------------ the harness
class Arena:
    """One torch.empty of FAR + SLOT floats; view(shape) hands out [2, ...] views with batch stride FAR."""

    def __init__(self, device):
        self.buf = torch.empty(FAR + SLOT, dtype=torch.float32, device=device)
        self.off = 0

    def reset(self):
        self.off = 0

    def view(self, shape):
        assert shape[0] == 2, "far rows run B = 2"
        n = 1
        inner = []
        for s in reversed(shape[1:]):
            inner.insert(0, n)
            n *= s
        take = (n + 63) // 64 * 64   # 256-byte aligned starts: the vector paths stay engaged
        assert self.off + take <= SLOT, "the row's tensors exceed an arena slot"
        v = torch.as_strided(self.buf, tuple(shape), (FAR, *inner), self.off)
        self.off += take
        return v


class Placer:
    """What a row's function places its tensors through: `far` is the set of parameter names that get the
    far stride in this run; every other tensor is dense."""

    def __init__(self, far, arena_in: Arena, arena_out: Arena, device="cuda"):
        self.far, self.ain, self.aout, self.dev = set(far), arena_in, arena_out, device
        self.seen = set()
        arena_in.reset()
        arena_out.reset()

    def inp(self, param, t):
        """An input [2, ...] holding t's values; its batch stride goes to `param` (None: always dense)."""
        t = torch.as_tensor(t).to(self.dev)
        if param in self.far:
            v = self.ain.view(t.shape)
            v.copy_(t)
            self.seen.add(param)
            return v
        return t.contiguous()

    def out(self, param, shape, init=None):
        """An output [2, ...] (zeros, or init's values for a tensor updated in place)."""
        if param in self.far:
            v = self.aout.view(tuple(shape))
            self.seen.add(param)
        else:
            v = torch.empty(tuple(shape), dtype=torch.float32, device=self.dev)
        if init is None:
            v.zero_()
        else:
            v.copy_(torch.as_tensor(init).to(self.dev))
        return v


def rnd(seed, *shape, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def P(t):
    return None if t is None else t.data_ptr()


def stream():
    return torch.cuda.current_stream().cuda_stream


# ----------------------------------------------------------------------------------------------- rows
# name -> (owner, (parameters), fn(placer) -> tuple of output tensors).  A parameter that several tensors
# share (c_bs of sa_gru_zr: cz and cr) places all of them.
FAR_ROWS: Dict[str, Tuple[str, Tuple[str, ...], Callable]] = {}


def row(name, owner, params):
    def add(fn):
        FAR_ROWS[name] = (owner, tuple(params), fn)
        return fn
    return add


def _relu_copy(p):
    C, HW = 3, 35
    x = p.inp("in_bs", rnd(1, 2, C, HW))
    o = p.out("out_bs", (2, C, HW))
    N.call("sa_relu_copy", P(x), x.stride(0), 2, C, HW, P(o), o.stride(0), stream())
    return (o,)


row("relu_copy", "sa_relu_copy", ("in_bs", "out_bs"))(_relu_copy)


def _gru_zr(HW):
    def fn(p):
        C = 4
        xc = p.inp("xc_bs", rnd(2, 2, 3 * C, HW))
        hzr = p.inp("hzr_bs", rnd(3, 2, 2 * C, HW))
        cz, cr = p.inp("c_bs", rnd(4, 2, C, HW)), p.inp("c_bs", rnd(5, 2, C, HW))
        h = p.inp("h_bs", rnd(6, 2, C, HW))
        bx = p.inp(None, rnd(7, 3 * C))
        z, rh = p.out(None, (2, C, HW)), p.out(None, (2, C, HW))
        N.call("sa_gru_zr", P(xc), xc.stride(0), P(bx), P(hzr), hzr.stride(0), P(cz), P(cr), cz.stride(0), P(h),
               h.stride(0), 2, C, HW, P(z), P(rh), stream())
        return z, rh
    return fn


def _gru_out(HW, split, entry):
    def fn(p):
        C = 4
        xc = p.inp("xc_bs", rnd(8, 2, 3 * C, HW))
        qh = p.inp("qh_bs", rnd(9, 2, C, HW))
        qh2 = p.inp("qh_bs", rnd(10, 2, C, HW)) if split else None
        cq = p.inp("c_bs", rnd(11, 2, C, HW))
        z = p.inp(None, torch.sigmoid(rnd(12, 2, C, HW)))
        bx = p.inp(None, rnd(13, 3 * C))
        h = p.out("h_bs", (2, C, HW), init=rnd(14, 2, C, HW))
        if entry == "sa_gru_out":
            N.call("sa_gru_out", P(xc), xc.stride(0), P(bx), P(qh), qh.stride(0), P(cq), cq.stride(0), P(z), 2, C, HW,
                   P(h), h.stride(0), stream())
        else:
            N.call("sa_gru_out_split", P(xc), xc.stride(0), P(bx), P(qh), P(qh2), qh.stride(0), P(cq), cq.stride(0),
                   P(z), 2, C, HW, P(h), h.stride(0), stream())
        return (h,)
    return fn


for _hw, _tag in ((36, "float4"), (35, "scalar")):
    row(f"gru_zr[{_tag}]", "sa_gru_zr", ("xc_bs", "hzr_bs", "c_bs", "h_bs"))(_gru_zr(_hw))
    row(f"gru_out[{_tag}]", "sa_gru_out", ("xc_bs", "qh_bs", "c_bs", "h_bs"))(_gru_out(_hw, False, "sa_gru_out"))
    row(f"gru_out_split[{_tag}]", "sa_gru_out_split", ("xc_bs", "qh_bs", "c_bs", "h_bs"))(
        _gru_out(_hw, True, "sa_gru_out_split"))


def _flow_update(p):
    H, W = 5, 9
    cx = p.out(None, (2, H * W), init=rnd(15, 2, H * W, scale=4.0))
    delta = p.inp("delta_bs", rnd(16, 2, 2, H, W))
    fa, fb = p.out("flow_a_bs", (2, 2, H, W)), p.out("flow_b_bs", (2, 2, H, W))
    N.call("sa_flow_update", P(cx), P(delta), delta.stride(0), 2, H, W, P(fa), fa.stride(0), P(fb), fb.stride(0),
           stream())
    return cx, fa, fb


row("flow_update", "sa_flow_update", ("delta_bs", "flow_a_bs", "flow_b_bs"))(_flow_update)


def _resample(entry, H, W, pad):
    """pool2x / interp, plain (pad 0) or pitched (rows pad floats wider than the width)."""
    pool = "pool2x" in entry

    def fn(p):
        C = 3
        Ho, Wo = ((H - 1) // 2 + 1, (W - 1) // 2 + 1) if pool else (2 * H - 1, 2 * W)
        x = rnd(17, 2, C, H, W + pad)
        x[..., W:] = 0
        x = p.inp("in_bs", x)
        o = p.out("out_bs", (2, C, Ho, Wo + pad))
        a = [P(x), x.stride(0)] + ([W + pad] if pad else []) + [2, C, H, W] + ([] if pool else [Ho, Wo])
        a += [P(o), o.stride(0)] + ([Wo + pad] if pad else [])
        N.call(entry, *a, stream())
        return (o,)
    return fn


row("pool2x[float4]", "sa_pool2x", ("in_bs", "out_bs"))(_resample("sa_pool2x", 10, 16, 0))
row("pool2x[scalar]", "sa_pool2x", ("in_bs", "out_bs"))(_resample("sa_pool2x", 7, 9, 0))
row("pool2x_p", "sa_pool2x_p", ("in_bs", "out_bs"))(_resample("sa_pool2x_p", 7, 14, 2))
row("interp[band]", "sa_interp_bilinear_ac", ("in_bs", "out_bs"))(_resample("sa_interp_bilinear_ac", 6, 10, 0))
row("interp_p", "sa_interp_bilinear_ac_p", ("in_bs", "out_bs"))(_resample("sa_interp_bilinear_ac_p", 6, 10, 4))


def _resample_multi(p):
    """Three jobs in one launch (pool2x, interp, flow planes), every job's two strides far or dense together."""
    C, H, W = 3, 8, 12
    jobs = (N.SaResampleJob * 3)()
    xs = [p.inp("in_bs", rnd(18 + i, 2, c, H, W)) for i, c in enumerate((C, C, 1))]
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    shapes = [(2, C, Ho, Wo), (2, C, 2 * H, 2 * W), (2, 2, H, W)]
    outs = [p.out("out_bs", s) for s in shapes]
    for i, (x, o, s) in enumerate(zip(xs, outs, shapes)):
        j = jobs[i]
        j.kind, j.B, j.C, j.H, j.W = i, 2, x.shape[1], H, W
        j.Ho, j.Wo = (H, W) if i == 2 else s[2:]
        j.in_, j.in_bs, j.in_pitch = x.data_ptr(), x.stride(0), W
        j.out, j.out_bs, j.out_pitch = o.data_ptr(), o.stride(0), j.Wo
    N.call("sa_resample_multi", 3, ctypes.addressof(jobs), stream())
    return tuple(outs)


row("resample_multi", "SaResampleJob", ("in_bs", "out_bs"))(_resample_multi)


def _softlrc(p):
    H, W = 5, 24
    d2, d3 = (p.inp("map_bs", rnd(21 + i, 2, H, W, scale=3.0).abs()) for i in range(2))
    c2, c3 = (p.inp("map_bs", torch.sigmoid(rnd(23 + i, 2, H, W))) for i in range(2))
    s2, s3 = p.out("map_bs", (2, H, W)), p.out("map_bs", (2, H, W))
    N.call("sa_softlrc", P(d2), P(d3), P(c2), P(c3), 2, H, W, d2.stride(0), 1.0, P(s2), P(s3), stream())
    return s2, s3


row("softlrc", "sa_softlrc", ("map_bs",))(_softlrc)


def _mono_scale_mirror(p):
    H, W = 5, 24
    m2, m3 = (p.inp("in_bs", rnd(25 + i, 2, H, W).abs()) for i in range(2))
    dL = p.inp("in_bs", rnd(27, 2, H, W, scale=3.0).abs())
    cf = p.inp("in_bs", torch.sigmoid(rnd(28, 2, H, W)))
    scale, shift = p.inp(None, torch.tensor([2.0, 3.0])), p.inp(None, torch.tensor([0.5, 0.25]))
    outs = [p.out(None, (2, H, W)) for _ in range(4)]
    N.call("sa_mono_scale_mirror", P(m2), P(m3), P(scale), P(shift), P(dL), P(cf), 2, H, W, m2.stride(0), 1.0, 0.5,
           *(P(o) for o in outs), stream())
    return tuple(outs)


row("mono_scale_mirror", "sa_mono_scale_mirror", ("in_bs",))(_mono_scale_mirror)


def _convex_upsample(p):
    H, W, f = 5, 8, 4
    flow = p.inp(None, rnd(29, 2, 1, H, W, scale=3.0))
    mask = p.inp("mask_bs", rnd(30, 2, 9 * f * f, H, W))
    o = p.out(None, (2, 1, f * H, f * W))
    N.call("sa_convex_upsample", P(flow), P(mask), mask.stride(0), 2, H, W, f, P(o), stream())
    return (o,)


row("convex_upsample", "sa_convex_upsample", ("mask_bs",))(_convex_upsample)


def _convex_upsample_backward(p):
    H, W, f = 5, 8, 4
    flow = p.inp(None, rnd(31, 2, 1, H, W, scale=3.0))
    mask = p.inp("mask_bs", rnd(32, 2, 9 * f * f, H, W))
    g = p.inp(None, rnd(33, 2, 1, f * H, f * W))
    gf, gm = p.out(None, (2, 1, H, W)), p.out(None, (2, 9 * f * f, H, W))
    N.call("sa_convex_upsample_backward", P(flow), P(mask), mask.stride(0), P(g), 2, H, W, f, float(f), P(gf), P(gm),
           stream())
    return gf, gm


row("convex_upsample_backward", "sa_convex_upsample_backward", ("mask_bs",))(_convex_upsample_backward)


def _conv2d_small(Cin):
    def fn(p):
        H, W, Cout, k = 9, 13, 64, 7
        x = p.inp("in_bs", rnd(34, 2, Cin, H, W))
        w, b = p.inp(None, rnd(35, Cout * Cin * k * k, scale=0.1)), p.inp(None, rnd(36, Cout))
        o = p.out("out_bs", (2, Cout, H, W))
        N.call("sa_conv2d_small", P(x), x.stride(0), 2, Cin, H, W, P(w), P(b), Cout, k, 1, P(o), o.stride(0),
               stream())
        return (o,)
    return fn


row("conv2d_small[2 channels, MFMA]", "sa_conv2d_small", ("in_bs", "out_bs"))(_conv2d_small(2))
row("conv2d_small[3 channels]", "sa_conv2d_small", ("in_bs", "out_bs"))(_conv2d_small(3))


def _conv2d_k3_narrow(p):
    Cin, H, W = 32, 9, 13
    x = p.inp("in_bs", rnd(37, 2, Cin, H, W))
    w, b = p.inp(None, rnd(38, 2 * Cin * 9, scale=0.1)), p.inp(None, rnd(39, 2))
    o = p.out("out_bs", (2, 2, H, W))
    N.call("sa_conv2d_k3_narrow", P(x), x.stride(0), 2, Cin, H, W, P(w), P(b), 2, P(o), o.stride(0), stream())
    return (o,)


row("conv2d_k3_narrow", "sa_conv2d_k3_narrow", ("in_bs", "out_bs"))(_conv2d_k3_narrow)


def _norm_act(HW):
    def fn(p):
        C = 3
        x, skip = p.inp("x_bs", rnd(40, 2, C, HW)), p.inp("skip_bs", rnd(41, 2, C, HW))
        m, s, t = (p.inp(None, rnd(42 + i, C)) for i in range(3))
        o = p.out("out_bs", (2, C, HW))
        N.call("sa_norm_act", P(x), x.stride(0), 2, C, HW, P(m), P(s), P(t), 0, 1, P(skip), skip.stride(0), None, None,
               None, 0, 0, 1, P(o), o.stride(0), stream())
        return (o,)
    return fn


row("norm_act[float4]", "sa_norm_act", ("x_bs", "skip_bs", "out_bs"))(_norm_act(36))
row("norm_act[scalar]", "sa_norm_act", ("x_bs", "skip_bs", "out_bs"))(_norm_act(35))


def _plane_stats(p):
    C, HW = 3, 36
    x = p.inp("x_bs", rnd(45, 2, C, HW))
    mean, rstd = p.out(None, (2, C)), p.out(None, (2, C))
    N.call("sa_plane_stats", P(x), x.stride(0), 2, C, HW, 1e-5, P(mean), P(rstd), stream())
    return mean, rstd


row("plane_stats", "sa_plane_stats", ("x_bs",))(_plane_stats)


def _softargmin(mode):
    def fn(p):
        H, n = 3, 64
        vd, vc = (p.inp("sb", rnd(46 + i, 2, n, H, n, scale=4.0)) for i in range(2))   # [B, W2, H, W1]
        outs = [p.out("out_bs", (2, H, n)) for _ in range(4)]
        N.lib().sa_softargmin_set_one_pass(mode)
        try:
            N.call("sa_softargmin_conf", P(vd), P(vc), 2, H, n, n, vd.stride(0), n, 1, H * n, *(P(o) for o in outs),
                   outs[0].stride(0), stream())
        finally:
            N.lib().sa_softargmin_set_one_pass(1)
        return tuple(outs)
    return fn


for _mode, _tag in ((1, "one pass"), (0, "line kernels")):
    row(f"softargmin_conf[{_tag}]", "sa_softargmin_conf", ("sb", "out_bs"))(_softargmin(_mode))


def _softargmin_backward(p):
    H, n = 3, 64
    vd, vc = (p.inp("sb", rnd(48 + i, 2, H, n, n, scale=4.0)) for i in range(2))   # [B, H, W1, W2]: sk == 1
    g = [p.inp(None, rnd(50 + i, 2, H, n)) for i in range(4)]
    gd, gc = p.out("sb", (2, H, n, n)), p.out("sb", (2, H, n, n))
    ws_bytes = int(N.lib().sa_softargmin_conf_backward_ws_size(2, H, n, n))
    ws = torch.empty(ws_bytes // 8 + 1, dtype=torch.float64, device=p.dev)
    N.call("sa_softargmin_conf_backward", P(vd), P(vc), 2, H, n, n, vd.stride(0), n * n, n, 1, *(P(t) for t in g),
           P(gd), P(gc), P(ws), stream())
    return gd, gc


row("softargmin_conf_backward", "sa_softargmin_conf_backward", ("sb",))(_softargmin_backward)


def _pyramid(vol_rows, W2, L):
    """The row-layout pyramid of dense rows [rows, W2] (sa_corr_pyramid_from_volume)."""
    rs = int(N.lib().sa_pyramid_row_stride(W2, L))
    pyr = torch.zeros((vol_rows.shape[0], rs), dtype=torch.float32, device=vol_rows.device)
    N.call("sa_corr_pyramid_from_volume", P(vol_rows), vol_rows.shape[0], W2, W2, L, P(pyr), rs, stream())
    return pyr, rs


def _lookup(kind, L, r):
    def fn(p):
        H, W = 5, 72
        K = L * (2 * r + 1)
        pa, rs = _pyramid(p.inp(None, rnd(52, 2 * H * W, W)), W, L)
        pb, _ = _pyramid(p.inp(None, rnd(53, 2 * H * W, W)), W, L)
        cx = p.inp("coords_bstride", torch.rand(2, 1, H, W, generator=torch.Generator().manual_seed(54)) * (W + 40) - 20)
        if kind == "lookup":
            o = p.out("out_bstride", (2, 2 * K, H, W))
            N.call("sa_corr_lookup", P(pa), P(pb), W, rs, L, r, P(cx), cx.stride(0), 2, H, W, P(o), o.stride(0), stream())
            return (o,)
        wt, bias = p.inp(None, rnd(55, K, 64, scale=0.2)), p.inp(None, rnd(56, 64))
        o = p.out(None, (4, 64, H, W))
        if kind == "fused":
            N.call("sa_corr_lookup_conv1x1", P(pa), P(pb), W, rs, L, r, P(cx), cx.stride(0), 2, H, W, P(wt), P(bias), 64,
                   P(o), stream())
            return (o,)
        assert N.lib().sa_corr_shear_supported(2, H, W, W, L) == 1
        sl = int(N.lib().sa_shear_slice_size(W, W, L))
        sh = [torch.zeros((2 * H, sl), dtype=torch.float32, device=p.dev) for _ in range(2)]
        for s, py in zip(sh, (pa, pb)):
            N.call("sa_corr_pyramid_shear", P(py), rs, 2, H, W, W, L, P(s), stream())
        N.call("sa_corr_lookup_conv1x1_sheared", P(sh[0]), P(sh[1]), W, L, r, P(cx), cx.stride(0), 2, H, W, P(wt),
               P(bias), 64, P(o), stream())
        return (o,)
    return fn


row("corr_lookup", "sa_corr_lookup", ("coords_bstride", "out_bstride"))(_lookup("lookup", 4, 4))
row("corr_lookup_conv1x1[4 levels, radius 4]", "sa_corr_lookup_conv1x1", ("coords_bstride",))(_lookup("fused", 4, 4))
row("corr_lookup_conv1x1[3 levels, radius 2]", "sa_corr_lookup_conv1x1", ("coords_bstride",))(_lookup("fused", 3, 2))
row("corr_lookup_conv1x1_sheared[4 levels, radius 4]", "sa_corr_lookup_conv1x1_sheared", ("coords_bstride",))(
    _lookup("sheared", 4, 4))
row("corr_lookup_conv1x1_sheared[3 levels, radius 2]", "sa_corr_lookup_conv1x1_sheared", ("coords_bstride",))(
    _lookup("sheared", 3, 2))


def _lookup_backward(p):
    H, W, L, r = 5, 72, 4, 4
    K = L * (2 * r + 1)
    g = p.inp("grad_bstride", rnd(57, 2, K, H, W))
    cx = p.inp("coords_bstride", torch.rand(2, 1, H, W, generator=torch.Generator().manual_seed(58)) * (W + 40) - 20)
    rs = int(N.lib().sa_pyramid_row_stride(W, L))
    o = p.out(None, (2, H * W * rs))
    N.call("sa_corr_lookup_backward", P(g), g.stride(0), P(cx), cx.stride(0), 2, H, W, W, L, r, P(o), rs, stream())
    return (o,)


row("corr_lookup_backward", "sa_corr_lookup_backward", ("grad_bstride", "coords_bstride"))(_lookup_backward)


def _from_volume_strided(sheared):
    def fn(p):
        H, W1, W2, L = 3, 36, 44, 4
        vol = p.inp("sb", rnd(59, 2, W2, H, W1))   # the hourglass's [B, W2, H, W1]
        if sheared:
            sl = int(N.lib().sa_shear_slice_size(W1, W2, L))
            o = p.out(None, (2, H * sl))
            N.call("sa_corr_pyramid_from_volume_strided_sheared", P(vol), 2, H, W1, W2, vol.stride(0), W1, H * W1, L,
                   P(o), stream())
        else:
            rs = int(N.lib().sa_pyramid_row_stride(W2, L))
            o = p.out(None, (2, H * W1 * rs))
            N.call("sa_corr_pyramid_from_volume_strided", P(vol), 2, H, W1, W2, vol.stride(0), W1, H * W1, L, P(o), rs,
                   stream())
        return (o,)
    return fn


row("pyramid_from_volume_strided", "sa_corr_pyramid_from_volume_strided", ("sb",))(_from_volume_strided(False))
row("pyramid_from_volume_strided_sheared", "sa_corr_pyramid_from_volume_strided_sheared", ("sb",))(
    _from_volume_strided(True))


def _two_row(entry):
    """Row strides: two rows FAR floats apart (the batch axis of the placer is the row axis here)."""
    def fn(p):
        W2, L = 44, 4
        rs = int(N.lib().sa_pyramid_row_stride(W2, L))
        if entry == "sa_corr_pyramid_from_volume":
            v = p.inp("in_row_stride", rnd(60, 2, W2))
            o = p.out("row_stride", (2, rs))
            N.call(entry, P(v), 2, W2, max(v.stride(0), W2), L, P(o), max(o.stride(0), rs), stream())
        elif entry == "sa_corr_pyramid_backward":
            g = p.inp("row_stride", rnd(61, 2, rs))
            o = p.out("out_row_stride", (2, W2))
            N.call(entry, P(g), 2, W2, g.stride(0), L, P(o), o.stride(0), stream())
        elif entry == "sa_corr_volume_pyramid":   # B 1, H 1, W1 2: two pyramid rows
            C = 16
            f2, f3 = p.inp(None, rnd(62, 1, C, 1, 2)), p.inp(None, rnd(63, 1, C, 1, W2))
            o = p.out("row_stride", (2, rs))
            N.call(entry, P(f2), P(f3), 1, C, 1, 2, W2, 4.0, None, None, 0.9, L, P(o), o.stride(0), stream())
        else:   # sa_corr_volume_backward: B 1, H 1, W1 2
            C = 16
            f2, f3 = p.inp(None, rnd(64, 1, C, 1, 2)), p.inp(None, rnd(65, 1, C, 1, W2))
            g = p.inp("vol_row_stride", rnd(66, 2, W2))
            g2, g3 = p.out(None, (2, C)), p.out(None, (2, C * W2 // 2))
            N.call(entry, P(g), g.stride(0), P(f2), P(f3), 1, C, 1, 2, W2, 4.0, P(g2), P(g3), stream())
            return g2, g3
        return (o,)
    return fn


row("pyramid_from_volume[two rows]", "sa_corr_pyramid_from_volume", ("in_row_stride", "row_stride"))(
    _two_row("sa_corr_pyramid_from_volume"))
row("pyramid_backward[two rows]", "sa_corr_pyramid_backward", ("row_stride", "out_row_stride"))(
    _two_row("sa_corr_pyramid_backward"))
row("corr_volume_pyramid[two rows]", "sa_corr_volume_pyramid", ("row_stride",))(_two_row("sa_corr_volume_pyramid"))
row("corr_volume_backward[two rows]", "sa_corr_volume_backward", ("vol_row_stride",))(
    _two_row("sa_corr_volume_backward"))


# ---- the 1x1 family, the direct convs, the Winograd convs and their epilogues, the tiler: weights and tables
# come from the ops module's own transforms (dense, shared by the dense and the far run)
def _weight(seed, cout, cin, k):
    return rnd(seed, cout, cin, k, k, scale=0.1).cuda()


def _conv1x1(Cin):
    def fn(p):
        from stereoanywhere_amd import ops
        Cout, H, W = 48, 6, 10
        x = p.inp("x_bs", rnd(70, 2, Cin, H, W))
        ws, bias = ops.conv1x1_weights(_weight(71, Cout, Cin, 1)), p.inp(None, rnd(72, Cout))
        o = p.out("out_bs", (2, Cout, H, W))
        N.call("sa_conv1x1", P(x), x.stride(0), 2, Cin, H, W, P(ws), Cout, P(bias), 0.25, P(o), o.stride(0), stream())
        return (o,)
    return fn


row("conv1x1[64 channels]", "sa_conv1x1", ("x_bs", "out_bs"))(_conv1x1(64))
row("conv1x1[96 channels]", "sa_conv1x1", ("x_bs", "out_bs"))(_conv1x1(96))


def _mask_upsample(p):
    from stereoanywhere_amd import ops
    Cin, H, W = 64, 5, 7
    x = p.inp("x_bs", rnd(73, 2, Cin, H, W))
    ws, bias = ops.conv1x1_weights(_weight(74, 144, Cin, 1)), p.inp(None, rnd(75, 144))
    flow = p.inp(None, rnd(76, 2, 1, H, W, scale=3.0))
    o = p.out("out_bs", (2, 1, 4 * H, 4 * W))
    N.call("sa_mask_upsample", P(x), x.stride(0), 2, Cin, H, W, P(ws), P(bias), 0.25, P(flow), P(o), o.stride(0),
           stream())
    return (o,)


row("mask_upsample", "sa_mask_upsample", ("x_bs", "out_bs"))(_mask_upsample)


def _conv_direct(form, split):
    """form: stem (7x7, 3 -> 64), stage (3x3 stride 2 + its 1x1 downsample, 16 -> 96), close (the stage conv on
    relu(relu((c2 - mean) rstd) + skip))."""
    def fn(p):
        from stereoanywhere_amd import ops
        if form == "stem":
            K, S, Cin, Cout, H, W = 7, 1, 3, 64, 9, 13
        else:
            K, S, Cin, Cout, H, W = 3, 2, 16, 96, 10, 14
        Ho, Wo = (H + 2 * (K // 2) - K) // S + 1, (W + 2 * (K // 2) - K) // S + 1
        wg = ops.conv_direct_weights(_weight(77, Cout, Cin, K), S, split=split)
        wd = None if form == "stem" else ops.conv_direct_weights(_weight(78, Cout, Cin, 1), S, with_ds=True, split=split)
        x = p.inp("c2_bs" if form == "close" else "in_bs", rnd(79, 2, Cin, H, W))
        o = p.out("out_bs", (2, Cout, Ho, Wo))
        ods = None if form == "stem" else p.out("out_ds_bs", (2, Cout, Ho, Wo))
        tail = [P(wg), P(wd), Cout, P(o), o.stride(0), P(ods), 0 if ods is None else ods.stride(0), None, None, stream()]
        if form == "close":
            skip = p.inp("skip_bs", rnd(80, 2, Cin, H, W))
            mean, rstd = p.inp(None, rnd(81, 2 * Cin, scale=0.2)), p.inp(None, rnd(82, 2 * Cin).abs() + 0.5)
            N.call("sa_conv_direct_close", P(x), x.stride(0), P(skip), skip.stride(0), P(mean), P(rstd), 2, Cin, H, W, K,
                   S, *tail[:2], int(split), *tail[2:])
        else:
            N.call("sa_conv_direct_split" if split else "sa_conv_direct", P(x), x.stride(0), 2, Cin, H, W, K, S, *tail)
        return (o,) if ods is None else (o, ods)
    return fn


for _split, _entry in ((False, "sa_conv_direct"), (True, "sa_conv_direct_split")):
    row(f"{_entry[3:]}[stem]", _entry, ("in_bs", "out_bs"))(_conv_direct("stem", _split))
    row(f"{_entry[3:]}[stride 2 + downsample]", _entry, ("in_bs", "out_bs", "out_ds_bs"))(_conv_direct("stage", _split))
    row(f"conv_direct_close[{'split' if _split else 'plain'}]", "sa_conv_direct_close",
        ("c2_bs", "skip_bs", "out_bs", "out_ds_bs"))(_conv_direct("close", _split))


def _wino2(entry):
    def fn(p):
        from stereoanywhere_amd import ops
        Cin, Cout, H, W = 8, 32, 6, 10
        U = ops.wino_weights(_weight(83, Cout, Cin, 3))
        bias = p.inp(None, rnd(84, Cout))
        q = "SaWinoProblem." if entry == "sa_conv2d_k3_wino_multi" else ""
        x = p.inp(q + "in_bs", rnd(85, 2, Cin, H, W))
        o = p.out(q + "out_bs", (2, Cout, H, W))
        if entry == "sa_conv2d_k3_wino":
            N.call(entry, P(x), x.stride(0), 2, Cin, H, W, P(U.u2), Cout, P(bias), 1, P(o), o.stride(0), stream())
        elif entry == "sa_conv2d_k3_wino_ex":
            m, sc, t = (p.inp(None, rnd(86 + i, Cin, scale=0.3)) for i in range(3))
            N.call(entry, P(x), x.stride(0), 2, Cin, H, W, P(U.u2), Cout, P(bias), 1, P(m), P(sc), P(t), 0, 1, P(o),
                   o.stride(0), None, stream())
        else:
            prob, _ = ops._wino_problem(x, U, bias, True, out=o, f4=False)
            arr = (N.SaWinoProblem * 1)(prob)
            N.call(entry, 1, ctypes.addressof(arr), stream())
        return (o,)
    return fn


row("conv2d_k3_wino", "sa_conv2d_k3_wino", ("in_bs", "out_bs"))(_wino2("sa_conv2d_k3_wino"))
row("conv2d_k3_wino_ex", "sa_conv2d_k3_wino_ex", ("in_bs", "out_bs"))(_wino2("sa_conv2d_k3_wino_ex"))
row("conv2d_k3_wino_multi", "SaWinoProblem", ("SaWinoProblem.in_bs", "SaWinoProblem.out_bs"))(
    _wino2("sa_conv2d_k3_wino_multi"))


def _wino4(shape, mode):
    """F(4x4): block shapes 0, 2 (fp32 products), 6 (split), 7 (single-f16 inputs); mode 0 the residual
    epilogue (skip), 1 / 2 the ConvGRU gates, 3 the flow head's partial sums."""
    W_, G_ = "SaWinoProblem.", "SaGateEpilogue."

    def fn(p):
        from stereoanywhere_amd import ops
        Ch, H, W = 32, 8, 16
        Cin, Cout = (2 * Ch, 2 * Ch) if mode == 1 else (Ch, Ch)
        U = ops.wino_weights(_weight(90, Cout, Cin, 3))
        bias = p.inp(None, rnd(91, Cout))
        x = p.inp(W_ + "in_bs", rnd(92, 2, Cin, H, W))
        split = shape in (6, 7)
        gates = (N.SaGateEpilogue * 1)()
        if mode == 0:
            skip = p.inp(W_ + "skip_bs", rnd(93, 2, Cout, H, W))
            o = p.out(W_ + "out_bs", (2, Cout, H, W))
            prob, _ = ops._wino_problem(x, U, bias, True, out=o, f4=True, split=split, skip=skip, skip_act="relu",
                                        out_act="relu")
            outs = (o,)
        elif mode == 3:
            per = int(N.lib().sa_flow_head_part_size(1, Cout, H, W))
            part = p.out(G_ + "head_part_bs", (2, per))
            head_w = p.inp(None, rnd(94, Cout * 9, scale=0.1))
            Uf = U.u4s if split else U.u4
            prob = N.SaWinoProblem(x.data_ptr(), x.stride(0), 2, Cin, H, W, Uf.data_ptr(), Cout, P(bias), 1, None, None,
                                   None, 0, 0, part.data_ptr(), 0, None, 0)
            gates[0].mode, gates[0].head_w, gates[0].head_part = 3, head_w.data_ptr(), part.data_ptr()
            gates[0].head_part_bs = part.stride(0)
            outs = (part,)
        else:
            ctx = p.inp(G_ + "ctx_bs", rnd(95, 2, Cout, H, W))
            h = p.inp(G_ + "h_bs", rnd(96, 2, Ch, H, W))
            o = p.out(W_ + "out_bs", (2, Ch, H, W))
            if mode == 1:
                o2 = p.out(G_ + "out2_bs", (2, Ch, H, W))
                gate, outs = dict(mode=1, ctx=ctx, h=h, out2=o2), (o, o2)
            else:
                z = p.inp(G_ + "z_bs", torch.sigmoid(rnd(97, 2, Ch, H, W)))
                add = p.inp(G_ + "add_bs", rnd(98, 2, Ch, H, W))
                gate, outs = dict(mode=2, ctx=ctx, h=h, z=z, add=add), (o,)
            prob, _ = ops._wino_problem(x, U, bias, False, out=o, f4=True, split=split,
                                        out_cout=Ch if mode == 1 else None)
            gates[0] = ops._gate_epilogue(dict(x=x, U=U, gate=gate))
        arr = (N.SaWinoProblem * 1)(prob)
        N.call("sa_conv2d_k3_wino4_launch", 1, ctypes.addressof(arr), ctypes.addressof(gates), shape,
               1 if split else 0, stream())
        return outs
    return fn


_W4 = {0: ("SaWinoProblem.in_bs", "SaWinoProblem.out_bs", "SaWinoProblem.skip_bs"),
       1: ("SaWinoProblem.in_bs", "SaWinoProblem.out_bs", "SaGateEpilogue.ctx_bs", "SaGateEpilogue.h_bs",
           "SaGateEpilogue.out2_bs"),
       2: ("SaWinoProblem.in_bs", "SaWinoProblem.out_bs", "SaGateEpilogue.ctx_bs", "SaGateEpilogue.h_bs",
           "SaGateEpilogue.z_bs", "SaGateEpilogue.add_bs"),
       3: ("SaWinoProblem.in_bs", "SaGateEpilogue.head_part_bs")}
for _shape in (0, 2, 6, 7):
    for _mode, _tag in ((0, "residual epilogue"), (1, "gate mode 1"), (2, "gate mode 2"), (3, "gate mode 3")):
        if (_shape, _mode) == (2, 3):   # refused: the flow-head epilogue needs the 8-wave shapes 0, 6 or 7
            continue
        row(f"conv2d_k3_wino4[block shape {_shape}, {_tag}]", "SaWinoProblem", _W4[_mode])(_wino4(_shape, _mode))


def _flow_head_reduce(p):
    Cout, H, W = 32, 8, 16
    per = int(N.lib().sa_flow_head_part_size(1, Cout, H, W))
    part, bias0 = p.inp(None, rnd(99, 2 * per)), p.inp(None, rnd(100, 1))
    cx = p.out(None, (2, H * W), init=rnd(101, 2, H * W, scale=4.0))
    fa, fb = p.out("flow_a_bs", (2, 2, H, W)), p.out("flow_b_bs", (2, 2, H, W))
    N.call("sa_flow_head_reduce", P(part), 2, Cout, H, W, P(bias0), P(cx), P(fa), fa.stride(0), P(fb), fb.stride(0),
           stream())
    return cx, fa, fb


row("flow_head_reduce", "sa_flow_head_reduce", ("flow_a_bs", "flow_b_bs"))(_flow_head_reduce)


def _feature_gates(p):
    C, H, W = 8, 6, 10
    x = p.inp("SaFeatureGateJob.in_bs", rnd(102, 2, H, W))
    w3, w1, b1 = (p.inp(None, rnd(103 + i, n, scale=0.3)) for i, n in enumerate((32 * 9, C * 32, C)))
    o = p.out("SaFeatureGateJob.out_bs", (2, C, H, W))
    jobs = (N.SaFeatureGateJob * 1)()
    j = jobs[0]
    j.in_, j.in_bs, j.B, j.H, j.W = x.data_ptr(), x.stride(0), 2, H, W
    j.w3, j.w1, j.b1, j.C, j.out, j.out_bs = w3.data_ptr(), w1.data_ptr(), b1.data_ptr(), C, o.data_ptr(), o.stride(0)
    ws = torch.empty(int(N.lib().sa_feature_gates_ws_size(1, ctypes.addressof(jobs))) // 8 + 1, dtype=torch.float64,
                     device=p.dev)
    N.call("sa_feature_gates", 1, ctypes.addressof(jobs), P(ws), stream())
    return (o,)


row("feature_gates", "SaFeatureGateJob", ("SaFeatureGateJob.in_bs", "SaFeatureGateJob.out_bs"))(_feature_gates)


def _tile_stitch(p):
    th, tw, H, W = 4, 6, 6, 8
    disp = p.inp("disp_ts", rnd(106, 2, th, tw))   # two slots
    tiles = torch.tensor([0, 0, 0, 2, 2, 1, 1, 1, 0], dtype=torch.int32, device=p.dev)
    wgt = p.inp(None, rnd(107, th * tw).abs() + 0.1)
    num, den = p.out(None, (2, H * W // 2)), p.out(None, (2, H * W // 2))
    N.call("sa_tile_stitch", P(disp), disp.stride(0), tw, P(tiles), 3, th, tw, P(wgt), H, W, 1, P(num), P(den), stream())
    return num, den


row("tile_stitch", "sa_tile_stitch", ("disp_ts",))(_tile_stitch)


def _softlrc_backward(p):
    H, W = 5, 24
    d2, d3 = (p.inp("map_bs", rnd(108 + i, 2, H, W, scale=3.0).abs()) for i in range(2))
    c2, c3 = (p.inp("map_bs", torch.sigmoid(rnd(110 + i, 2, H, W))) for i in range(2))
    g2, g3 = (p.inp("map_bs", rnd(112 + i, 2, H, W)) for i in range(2))
    outs = [p.out("map_bs", (2, H, W)) for _ in range(4)]
    ws = torch.empty(int(N.lib().sa_softlrc_backward_ws_size(2, H, W)) // 8 + 1, dtype=torch.float64, device=p.dev)
    N.call("sa_softlrc_backward", P(d2), P(d3), P(c2), P(c3), 2, H, W, d2.stride(0), 1.0, P(g2), P(g3),
           *(P(o) for o in outs), P(ws), stream())
    return tuple(outs)


row("softlrc_backward", "sa_softlrc_backward", ("map_bs",))(_softlrc_backward)


# ---- line and row strides: the placer's "batch" axis is the line (or pyramid row) that the stride separates
def _lookup_rows(kind, L, r):
    """Pyramids of two pixels (B 2, H 1, W1 1), their rows FAR floats apart."""
    def fn(p):
        W2 = 72
        K = L * (2 * r + 1)
        rs = int(N.lib().sa_pyramid_row_stride(W2, L))
        dense = [_pyramid(p.inp(None, rnd(120 + i, 2, W2)), W2, L)[0] for i in range(2)]
        pa, pb = (p.inp("row_stride", d) for d in dense)
        cx = p.inp(None, torch.tensor([[[[30.3]]], [[[69.6]]]]))
        if kind == "shear":   # B 1, H 1, W1 2
            sl = int(N.lib().sa_shear_slice_size(2, W2, L))
            o = p.out(None, (2, sl // 2))
            N.call("sa_corr_pyramid_shear", P(pa), pa.stride(0), 1, 1, 2, W2, L, P(o), stream())
        elif kind == "lookup":
            o = p.out(None, (2, 2 * K))
            N.call("sa_corr_lookup", P(pa), P(pb), W2, pa.stride(0), L, r, P(cx), 1, 2, 1, 1, P(o), 2 * K, stream())
        else:
            wt, bias = p.inp(None, rnd(122, K, 64, scale=0.2)), p.inp(None, rnd(123, 64))
            o = p.out(None, (4, 64))
            N.call("sa_corr_lookup_conv1x1", P(pa), P(pb), W2, pa.stride(0), L, r, P(cx), 1, 2, 1, 1, P(wt), P(bias), 64,
                   P(o), stream())
        return (o,)
    return fn


row("corr_lookup[two pixels]", "sa_corr_lookup", ("row_stride",))(_lookup_rows("lookup", 4, 4))
row("corr_lookup_conv1x1[two pixels, 4 levels, radius 4]", "sa_corr_lookup_conv1x1", ("row_stride",))(
    _lookup_rows("fused", 4, 4))
row("corr_lookup_conv1x1[two pixels, 3 levels, radius 2]", "sa_corr_lookup_conv1x1", ("row_stride",))(
    _lookup_rows("fused", 3, 2))
row("corr_pyramid_shear[two pixels]", "sa_corr_pyramid_shear", ("row_stride",))(_lookup_rows("shear", 4, 4))


def _strided_lines(which, sheared):
    """sa_corr_pyramid_from_volume_strided(_sheared) with B 1: sh far over H = 2 image rows, sk far over W2 = 2
    cells (one level)."""
    def fn(p):
        W1 = 36
        H, W2, L = (2, 44, 4) if which == "sh" else (1, 2, 1)
        v = p.inp(which, rnd(124, 2, W2 * W1 if which == "sh" else H * W1))
        sh, sk = (v.stride(0), W1) if which == "sh" else (W1, v.stride(0))
        if sheared:
            o = p.out(None, (2, H * int(N.lib().sa_shear_slice_size(W1, W2, L)) // 2))
            N.call("sa_corr_pyramid_from_volume_strided_sheared", P(v), 1, H, W1, W2, 4 * H * W1 * W2, sh, sk, L, P(o),
                   stream())
        else:
            rs = int(N.lib().sa_pyramid_row_stride(W2, L))
            o = p.out(None, (2, H * W1 * rs // 2))
            N.call("sa_corr_pyramid_from_volume_strided", P(v), 1, H, W1, W2, 4 * H * W1 * W2, sh, sk, L, P(o), rs,
                   stream())
        return (o,)
    return fn


def _strided_rows(p):
    """The output row stride of sa_corr_pyramid_from_volume_strided: W1 % 4 == 0 makes four pyramid rows the
    least (B 1, H 1, W1 4).  They sit FAR / 3 floats apart in the output arena, so the fourth starts FAR floats
    in: the offset 3 * row_stride crosses 2^31 elements and 2^33 bytes as a far batch offset does."""
    W1, W2, L = 4, 44, 4
    rs = int(N.lib().sa_pyramid_row_stride(W2, L))
    v = p.inp(None, rnd(130, 1, W2 * W1))
    if "row_stride" in p.far:
        assert FAR % 12 == 0 and 3 * (FAR // 3) == FAR
        o = torch.as_strided(p.aout.buf, (W1, rs), (FAR // 3, 1))
        p.seen.add("row_stride")
    else:
        o = torch.empty((W1, rs), dtype=torch.float32, device=p.dev)
    o.zero_()
    N.call("sa_corr_pyramid_from_volume_strided", P(v), 1, 1, W1, W2, 4 * W1 * W2, W1, W1, L, P(o), o.stride(0), stream())
    return (o,)


row("pyramid_from_volume_strided[four rows]", "sa_corr_pyramid_from_volume_strided", ("row_stride",))(_strided_rows)
for _which in ("sh", "sk"):
    row(f"pyramid_from_volume_strided[{_which}]", "sa_corr_pyramid_from_volume_strided", (_which,))(
        _strided_lines(_which, False))
    row(f"pyramid_from_volume_strided_sheared[{_which}]", "sa_corr_pyramid_from_volume_strided_sheared", (_which,))(
        _strided_lines(_which, True))


def _softargmin_lines(which, backward):
    """B 1; the far stride separates H = 2 image rows (sh), W1 = 2 left pixels (sj, sk = 1) or W2 = 2 right
    pixels (sk, sj = 1); the other two axes are dense inside a line."""
    def fn(p):
        n = 64
        H, W1, W2 = (2, n, n) if which == "sh" else (3, 2, n) if which == "sj" else (3, n, 2)
        inner = (W2, W1) if which == "sh" else (H, W2) if which == "sj" else (H, W1)   # [far axis][..][..]
        vd, vc = (p.inp(which, rnd(125 + i, 2, *inner, scale=4.0)) for i in range(2))
        far = vd.stride(0)
        sb = 4 * H * W1 * W2   # (B = 1: never multiplied by more than 0)
        sh, sj, sk = {"sh": (far, 1, W1), "sj": (W2, far, 1), "sk": (W1, 1, far)}[which]
        if not backward:
            m = max(W1, W2)
            outs = [p.out(None, (2, H * m // 2)) for _ in range(4)]
            N.call("sa_softargmin_conf", P(vd), P(vc), 1, H, W1, W2, sb, sh, sj, sk, *(P(o) for o in outs), H * m,
                   stream())
            return tuple(outs)
        g = [p.inp(None, rnd(127 + i, H * (W1 if i % 2 == 0 else W2))) for i in range(4)]   # g_dL, g_dR, g_cL, g_cR
        gd, gc = p.out(which, (2, *inner)), p.out(which, (2, *inner))
        ws = torch.empty(int(N.lib().sa_softargmin_conf_backward_ws_size(1, H, W1, W2)) // 8 + 1, dtype=torch.float64,
                         device=p.dev)
        N.call("sa_softargmin_conf_backward", P(vd), P(vc), 1, H, W1, W2, sb, sh, sj, sk, *(P(t) for t in g), P(gd),
               P(gc), P(ws), stream())
        return gd, gc
    return fn


for _which in ("sh", "sj", "sk"):
    row(f"softargmin_conf[{_which}]", "sa_softargmin_conf", (_which,))(_softargmin_lines(_which, False))
    row(f"softargmin_conf_backward[{_which}]", "sa_softargmin_conf_backward", (_which,))(_softargmin_lines(_which, True))


# -------------------------------------------------------------------------- refusals seen on the CPU
X, Y, Z = 1 << 20, 1 << 28, 1 << 34   # any non-null values: validation fails before a pointer is used
GATED: Dict[Tuple[str, str], Tuple[str, Callable, bytes]] = {
    ("sa_corr_lookup_backward", "row_stride"): (
        "stereoanywhere_amd/csrc/corr_backward.hip:242",
        lambda: N.lib().sa_corr_lookup_backward(X, 10000, Y, 100, 1, 4, 8, 64, 4, 4, Z, FAR, None),
        b"row_stride"),
}


# ----------------------------------------------------------------------------------------- the table
def _table():
    t = {}
    for name, (owner, params, _) in FAR_ROWS.items():
        for q in params:   # "Struct.field" names a field of another owner than the row's
            t.setdefault(tuple(q.split(".")) if "." in q else (owner, q), ("far", name))
    for key, (where, _, _) in GATED.items():
        t[key] = ("gated", where)
    return t


TABLE = _table()
