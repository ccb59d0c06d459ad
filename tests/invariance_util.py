"""Harness of tests/test_gpu_invariance.py: replica, rerun, dirty-memory and two-stream bit-equality.

A case (class Case) builds the inputs of ONE sample from a seeded generator and replicates them R
times along the batch with the `rep` it is handed; weights, tables and per-channel vectors are built
once and shared.  `call(inputs, dests)` launches the op and returns a tuple of output tensors whose
first dimension is the batch, cut to the documented extent of each output (a pyramid row's used
columns, not its padding).  `dests(inputs)` allocates whatever the case passes as `out=` or writes
in place; the harness fills those with the poison word before every call.  `oracle(inputs, outs)`
compares out[0] with the op's own float64 / oracle restatement at its own test's tolerance; `before(inputs)`
and `after(inputs)` run around the first poisoned launch (a process-global counter read and reset).

run_case checks, all on bits (integer views, so NaN != NaN hides nothing):
  P1  out[b] == out[0] for every replica b;
  P2  three calls give the same result;
  P3  those three calls run on memory poisoned with 0xFFFFFFFF words, then zeros, then 0xFFFFFFFF
      again: the destinations and the caching allocator's free blocks (poison_free_memory, which checks
      itself: a fresh torch.empty of the output's size must read back the word);
  P4  (cases with streams=True) the call on two side streams at once equals the serial result.
The oracle comparison is made on the first, NaN-poisoned result, so a finite oracle value also proves
that no poison leaked into it.
"""
from __future__ import annotations

from typing import Callable, Optional, Sequence

import torch

ONES, ZEROS = -1, 0   # int32 words 0xFFFFFFFF (NaN as f32 and as f64; 4 G as a counter) and 0
PATTERNS = (ONES, ZEROS, ONES)
_INT = {1: torch.int8, 2: torch.int16, 4: torch.int32, 8: torch.int64}
# sub-megabyte block sizes (bytes; the allocator's small pool serves requests up to 1 MiB), _PER_SIZE of each
_SMALL = (1 << 20, 512 << 10, 128 << 10, 32 << 10, 8 << 10, 2 << 10, 512)
_PER_SIZE = 4


class PoisonDidNotTake(AssertionError):
    pass


def bits(t: torch.Tensor) -> torch.Tensor:
    """The tensor's bytes as integers of its element size (contiguous copy of a view)."""
    t = t.detach().contiguous()
    return t if not t.is_floating_point() else t.view(_INT[t.element_size()])


def same_bits(a: torch.Tensor, b: torch.Tensor) -> bool:
    return a.shape == b.shape and a.dtype == b.dtype and torch.equal(bits(a), bits(b))


def fill_words(t: torch.Tensor, word: int) -> None:
    """Every 32-bit word of t's own elements becomes `word` (t may be a strided view; 2-byte types get
    the half word, 8-byte types the word twice)."""
    if t.is_floating_point():
        if t.is_contiguous():
            t.view(_INT[t.element_size()]).fill_(word)
        else:   # a view: write through an integer copy of the right shape
            t.copy_(torch.full(t.shape, word, dtype=_INT[t.element_size()], device=t.device).view(t.dtype))
    else:
        t.fill_(word)


def _free_blocks(device):
    """(pool, bytes) of every block the caching allocator holds free for the default stream."""
    index = torch.device(device).index
    index = torch.cuda.current_device() if index is None else index
    return [(seg["segment_type"], blk["size"]) for seg in torch.cuda.memory_snapshot()
            if seg["device"] == index and seg.get("stream", 0) == 0
            for blk in seg["blocks"] if blk["state"] == "inactive"]


def poison_free_memory(device, peak_bytes: int, probe_bytes: int, word: int) -> None:
    """Fill the caching allocator's free blocks with `word`.  One block of at least twice the call's peak
    allocation and a few dozen sub-megabyte blocks are allocated; then every block the allocator's own
    snapshot lists as free (the rests of the segments those came from, and of the segments the live
    tensors sit in) is allocated at its exact size; all are filled and freed.  Then the self-check: a
    torch.empty of probe_bytes must read back `word` everywhere, else PoisonDidNotTake (so that P3 cannot
    pass on memory nobody dirtied)."""
    torch.cuda.synchronize(device)
    torch.cuda.empty_cache()   # cached segments nobody uses go back: what is free afterwards is listed below

    def take(nbytes):
        return torch.empty(nbytes // 4, dtype=torch.int32, device=device)
    held = [take(max(2 * peak_bytes, 2 << 20))] + [take(size) for size in _SMALL for _ in range(_PER_SIZE)]
    for _ in range(4):   # (a request the cache could not serve brings a new segment: list again)
        sizes = []
        for pool, size in _free_blocks(device):
            while pool == "small" and size > _SMALL[0]:   # the small pool serves requests up to 1 MiB
                sizes.append(_SMALL[0])
                size -= _SMALL[0]
            sizes.append(size)
        if not sizes:
            break
        held += [take(size) for size in sorted(sizes, reverse=True)]
    for h in held:
        h.fill_(word)
    del held, h
    torch.cuda.synchronize(device)
    check_poison(device, probe_bytes, word)


def check_poison(device, probe_bytes: int, word: int) -> None:
    probe = torch.empty(max(probe_bytes, 4) // 4, dtype=torch.int32, device=device)
    bad = int((probe != word).sum())
    del probe
    if bad:
        raise PoisonDidNotTake(f"poison did not take: {bad} of {max(probe_bytes, 4) // 4} words of a fresh "
                               f"{probe_bytes}-byte allocation do not hold {word & 0xFFFFFFFF:#x}")


class Case:
    """One row of the invariance table; see the module docstring."""

    def __init__(self, name: str, inputs: Callable, call: Callable, oracle: Callable, *, R: int = 8,
                 dests: Optional[Callable] = None, streams: bool = False, before: Optional[Callable] = None,
                 after: Optional[Callable] = None, p1: bool = True):
        self.name, self.inputs, self.call, self.oracle = name, inputs, call, oracle
        self.R, self.dests, self.streams, self.before, self.after = R, dests, streams, before, after
        self.p1 = p1   # False: the op has no batch position to compare (the case says why); P2 to P4 stay

    def __repr__(self) -> str:
        return self.name


def replicator(R: int, device="cuda") -> Callable:
    """rep(x): the one sample x [1, ...] (CPU or GPU tensor, or numpy array) R times along the batch,
    contiguous on the device."""
    def rep(x):
        x = torch.as_tensor(x)
        assert x.shape[0] == 1, "a case builds one sample"
        return x.to(device).expand(R, *x.shape[1:]).contiguous()
    return rep


def _launch(case: Case, inp, word: Optional[int]):
    dests = case.dests(inp) if case.dests is not None else ()
    if word is not None:
        for d in dests:
            fill_words(d, word)
    outs = case.call(inp, dests)
    assert isinstance(outs, tuple) and outs, "call returns a tuple of output tensors"
    return outs


def _snapshot(outs: Sequence[torch.Tensor]):
    torch.cuda.synchronize()
    return tuple(bits(o).cpu() for o in outs)


def _assert_equal(label: str, a, b) -> None:
    for i, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and x.dtype == y.dtype, f"{label}: output {i} changed its shape"
        if not torch.equal(x, y):
            diff = x != y
            first = diff.nonzero()[0].tolist()
            raise AssertionError(f"{label}: output {i} differs in {int(diff.sum())} of {x.numel()} elements, "
                                 f"first at {first}: {int(x[tuple(first)]):#x} != {int(y[tuple(first)]):#x}")


def _assert_replicas(label: str, snap, R: int) -> None:
    for i, x in enumerate(snap):
        assert x.shape[0] == R, f"{label}: output {i} has batch {x.shape[0]}, not {R}"
        flat = x.reshape(R, -1)
        diff = (flat != flat[:1]).any(1)
        if diff.any():
            b = int(diff.nonzero()[0])
            col = int((flat[b] != flat[0]).nonzero()[0])
            distinct = len({row.numpy().tobytes() for row in flat})
            raise AssertionError(f"{label}: output {i}: {int(diff.sum())} of {R} replicas differ from replica 0 "
                                 f"({distinct} distinct results); replica {b}, element {col}: "
                                 f"{int(flat[b, col]):#x} != {int(flat[0, col]):#x}")


def run_case(case: Case, device="cuda") -> dict:
    """P1 to P4 and the oracle comparison of one case; returns the measurements it made."""
    dev = torch.device(device)
    inp = case.inputs(replicator(case.R, dev))
    torch.cuda.synchronize(dev)
    # the call's peak allocation, from a first, unpoisoned call
    torch.cuda.reset_peak_memory_stats(dev)
    base = torch.cuda.memory_allocated(dev)
    outs = _launch(case, inp, None)
    torch.cuda.synchronize(dev)
    peak = torch.cuda.max_memory_allocated(dev) - base
    serial = _snapshot(outs)
    probe = max(o.numel() * o.element_size() for o in outs)
    del outs
    snaps = []
    for k, word in enumerate(PATTERNS):
        poison_free_memory(dev, peak, probe, word)
        if k == 0 and case.before is not None:
            case.before(inp)
        outs = _launch(case, inp, word)
        if k == 0:
            torch.cuda.synchronize(dev)
            case.oracle(inp, outs)   # on the NaN-poisoned result
            if case.after is not None:
                case.after(inp)
        snaps.append(_snapshot(outs))
        del outs
    for k, s in enumerate(snaps if case.p1 else ()):
        _assert_replicas(f"{case.name} P1 (launch {k}, poison {PATTERNS[k] & 0xFFFFFFFF:#x})", s, case.R)
    _assert_equal(f"{case.name} P3 (all-ones vs zero poison)", snaps[0], snaps[1])
    _assert_equal(f"{case.name} P2 (first vs third launch)", snaps[0], snaps[2])
    _assert_equal(f"{case.name} P3 (unpoisoned vs poisoned)", serial, snaps[0])
    if case.streams:
        cur = torch.cuda.current_stream(dev)
        side = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
        res = []
        for s in side:
            s.wait_stream(cur)
        for s in side:   # both enqueued before either is waited for: they overlap on the device
            with torch.cuda.stream(s):
                res.append(_launch(case, inp, ONES))
        for s in side:
            s.synchronize()
        for k, r in enumerate(res):
            _assert_equal(f"{case.name} P4 (stream {k} vs serial)", _snapshot(r), serial)
        del res
    return {"peak_bytes": peak, "probe_bytes": probe}
