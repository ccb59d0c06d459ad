"""Replay of the whole test-mode forward from a hipGraph (torch.cuda.graph over the HIP kernels,
the few MIOpen calls and every side stream of the forward).

The forward has no host synchronisation and no data-dependent control flow, so one capture per
(input shapes, iterations, schedule, weight version) serves every later call: the inputs are
copied into the graph's static buffers and the graph is replayed.  The host then enqueues one
graph launch per forward instead of ~1.4k kernel launches, which is what lets the GRU loop's
batch parts (ScheduleOptions.loop_parts) overlap on the GPU without the host falling behind.
"""
from __future__ import annotations

import dataclasses
from typing import Optional

import torch


class ForwardGraph:
    """Callable like StereoAnywhere.forward(image2, image3, mde2, mde3, iters, test_mode=True);
    returns (flow_up, None) with flow_up a fresh tensor (the graph's output buffer is reused)."""

    def __init__(self, model: torch.nn.Module):
        self.model = model
        self._key = None
        self._graph: Optional[torch.cuda.CUDAGraph] = None
        self._static = None
        self._out = None
        # this instance's own capture stream (not torch's shared default capture stream).  The
        # captured launches hold no per-stream workspace: the split kernels' range guards recompute
        # an overflowed block inside its own launch, so graph instances replayed at the same time on
        # different streams (PipelinedForward) share no state
        self._cap_stream: Optional[torch.cuda.Stream] = None

    def _make_key(self, xs, iters):
        m = self.model
        m._weights()   # the derived weights of the current parameter version
        from . import encoders, ops
        from . import _native as N
        # everything that picks the captured kernels: the schedule, the module-level kernel
        # switches and the library's own A/B switches (set by A/B scripts and tests) and the
        # model's flags, and whether this call runs in mixed precision (a default capture is never
        # replayed for a mixed call, nor the reverse)
        args = tuple(sorted((k, repr(v)) for k, v in vars(m.args).items()))
        lib = N.lib()
        # (an A/B run's older library, SA_HIP_LIB, may lack a getter: its switch reads as None)
        c_switches = tuple(getattr(lib, name)() if hasattr(lib, name) else None
                           for name in ("sa_lookup_get_mfma", "sa_softargmin_get_one_pass", "sa_conv3d_wd_get_variant",
                                         "sa_conv3d_mf_get_planes",
                                         "sa_lookup_get_shear_dual"))
        return (tuple((tuple(x.shape), x.dtype, x.device) for x in xs), iters, dataclasses.astuple(m.opts),
                m.stream_overlap, m._derived_key, (ops._WINO4, ops.W4_SPLIT, ops.DIRECT_SPLIT, ops._WINO4_MIN_BLOCKS,
                                                   ops.SPLIT_GUARD, ops.CONV3D_MFMA, ops.CONV1X1,
                                                   encoders.FNET_LAZY_CLOSE, encoders.DIRECT_SMALL),
                c_switches, args, m.mixed_precision_active())

    def __call__(self, image2, image3, mde2, mde3, iters: int = 12, test_mode: bool = True):
        if not test_mode:
            raise NotImplementedError("ForwardGraph replays the test-mode forward only")
        xs = (image2, image3, mde2, mde3)
        with torch.no_grad():
            key = self._make_key(xs, iters)
            if key != self._key:
                self._capture(xs, iters)
                self._key = key
            for d, x in zip(self._static, xs):
                d.copy_(x)
            self._graph.replay()
            return self._out.clone(), None

    def _capture(self, xs, iters):
        self._graph = None
        self._static = [x.detach().clone() for x in xs]
        # one eager forward on a side stream first (derived weights, MIOpen plans, allocator
        # pools), as torch.cuda.graph requires
        cur = torch.cuda.current_stream()
        s = torch.cuda.Stream()
        s.wait_stream(cur)
        with torch.cuda.stream(s):
            self.model(*self._static, iters=iters, test_mode=True)
        cur.wait_stream(s)
        g = torch.cuda.CUDAGraph()
        if self._cap_stream is None:
            self._cap_stream = torch.cuda.Stream()
        with torch.cuda.graph(g, stream=self._cap_stream):
            self._out = self.model(*self._static, iters=iters, test_mode=True)[0]
        self._graph = g


class PipelinedForward:
    """``depth`` ForwardGraph instances (each with its own static buffers and memory pool) replayed
    round-robin on ``depth`` streams: consecutive forwards of independent batches are in flight
    together, so one batch's update loop overlaps the next batch's encoders and mono branch.
    Same results as ForwardGraph; a returned tensor is ready on its instance's stream (synchronise
    before reading it on another)."""

    def __init__(self, model: torch.nn.Module, depth: int = 2):
        if depth < 1:
            raise ValueError("PipelinedForward: depth >= 1")
        self.graphs = [ForwardGraph(model) for _ in range(depth)]
        self.streams = [torch.cuda.Stream() for _ in range(depth)]
        self._i = 0

    def __call__(self, image2, image3, mde2, mde3, iters: int = 12, test_mode: bool = True):
        i = self._i
        self._i = (i + 1) % len(self.graphs)
        s = self.streams[i]
        s.wait_stream(torch.cuda.current_stream())   # the inputs (and anything else queued before)
        with torch.cuda.stream(s):
            return self.graphs[i](image2, image3, mde2, mde3, iters=iters, test_mode=test_mode)
