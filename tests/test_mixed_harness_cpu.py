"""The harness wrappers hand ``mixed_precision`` to the wrapped model the way the reference does
(tile_wrapper.py:238, 305, tiled_inference.py:197, 306, cpu_offload_wrapper.py:66, 78): they call
it under torch.autocast of their device type exactly when the flag is set.  A stub model on the CPU
records what it saw; the wrappers accept any model, so autocast is the whole signal."""
import numpy as np
import pytest
import torch

from stereoanywhere_amd import tiler
from stereoanywhere_amd.offload import CPUOffloadWrapper


class Stub(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.seen = []

    def forward(self, l, r, ml=None, mr=None, iters=1, test_mode=True, **kw):
        self.seen.append(torch.is_autocast_enabled("cpu"))
        return -(l[:, :1] + 0.5 * r[:, 1:2]), None


class StubMono(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))
        self.seen = []

    def forward(self, l, r):
        self.seen.append(torch.is_autocast_enabled("cpu"))
        return l.mean(1, keepdim=True), r.mean(1, keepdim=True)


def _pair(h, w, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(1, 3, h, w, generator=g), torch.rand(1, 3, h, w, generator=g)


@pytest.mark.parametrize("batch_tiles", [False, True])
@pytest.mark.parametrize("h,w", [(96, 160), (64, 64)])   # tiled; fits one tile (the direct call)
def test_tile_wrapper_enters_autocast_when_asked(batch_tiles, h, w):
    l, r = _pair(h, w)
    m = torch.rand(1, 1, h, w)
    outs = {}
    for flag in (False, True):
        stub = Stub()
        tw = tiler.TileWrapper(stub, tile_size=64, overlap=32, batch_tiles=batch_tiles)
        outs[flag] = tw(l, r, m, m, mixed_precision=flag, iters=1, test_mode=True)
        assert stub.seen and all(s is flag for s in stub.seen), (flag, stub.seen)
        assert not torch.is_autocast_enabled("cpu")
    # the default is off
    stub = Stub()
    tiler.TileWrapper(stub, tile_size=64, overlap=32, batch_tiles=batch_tiles)(l, r, m, m, iters=1, test_mode=True)
    assert stub.seen and not any(stub.seen)
    assert outs[True].dtype == torch.float32 and torch.equal(outs[True], outs[False])


@pytest.mark.parametrize("flag", [False, True])
def test_mapreduce_guidance_and_tile_pass(flag):
    rng = np.random.default_rng(2)
    l = rng.integers(0, 256, (128, 192, 3), dtype=np.uint8)
    r = rng.integers(0, 256, (128, 192, 3), dtype=np.uint8)
    mono = (torch.rand(1, 1, 128, 192), torch.rand(1, 1, 128, 192))
    stub = Stub()
    inf = tiler.MapReduceInference(stub, tile_width=64, tile_height=64, overlap=32, use_global_guidance=True,
                                   mixed_precision=flag)
    d = inf.infer(l, r, mono_pair=mono, iters=1, test_mode=True)
    assert d.dtype == np.float32
    # the first call is the low-resolution guidance pass, the rest the tiles
    assert len(stub.seen) > 2 and all(s is flag for s in stub.seen), stub.seen
    assert not torch.is_autocast_enabled("cpu")


def test_offload_wrapper_reads_the_keyword():
    l, r = _pair(32, 64, seed=1)
    for kw, want in (({}, False), (dict(mixed_precision=False), False), (dict(mixed_precision=True), True)):
        stub, mono = Stub(), StubMono()
        CPUOffloadWrapper(stub, mono)(l, r, iters=1, test_mode=True, **kw)
        assert stub.seen == [want] and mono.seen == [want], (kw, stub.seen, mono.seen)
    assert not torch.is_autocast_enabled("cpu")
