"""NaN guard bands around kernel outputs, shared by the direct GPU tests (tests/test_gpu_rowwise.py,
tests/test_gpu_layernorm.py).

Every output a wrapper allocates is, for the duration of the call, a view into a larger NaN-filled buffer (``guarded``
stands in for torch.empty / torch.empty_like inside ops): the bands before and after must still be NaN afterwards.
Destinations the caller owns get the same bands from ``poisoned``."""
import contextlib
import math

import torch

GUARD = 64                                    # elements on each side: a multiple of 16 bytes in every dtype


class _GuardedTorch:
    """torch, except that empty / empty_like hand out the middle of a NaN-filled buffer"""

    def __init__(self):
        self.live = []

    def __getattr__(self, name):
        return getattr(torch, name)

    def empty(self, *shape, dtype=None, device=None, **kw):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list, torch.Size)):
            shape = tuple(shape[0])
        if dtype is None or not dtype.is_floating_point or device is None or torch.device(device).type != "cuda":
            return torch.empty(shape, dtype=dtype, device=device, **kw)
        n = math.prod(shape)
        buf = torch.full((n + 2 * GUARD,), math.nan, dtype=dtype, device=device)
        self.live.append((buf, n))
        return buf[GUARD:GUARD + n].view(shape)

    def empty_like(self, t, **kw):
        return self.empty(tuple(t.shape), dtype=kw.get("dtype", t.dtype), device=t.device)

    def check(self):
        assert self.live, "the call allocated no output"
        for buf, n in self.live:
            assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), "a guard band was written"


@contextlib.contextmanager
def guarded(ops):
    g = _GuardedTorch()
    ops.torch = g
    try:
        yield g
    finally:
        ops.torch = torch
    g.check()


def poisoned(shape, dtype, device, fill=math.nan):
    """(view, check): a caller-owned destination inside NaN bands; the view itself starts as ``fill``"""
    n = math.prod(shape)
    buf = torch.full((n + 2 * GUARD,), math.nan, dtype=dtype, device=device)
    view = buf[GUARD:GUARD + n].view(shape)
    view.fill_(fill)

    def check():
        assert bool(torch.isnan(buf[:GUARD]).all()) and bool(torch.isnan(buf[GUARD + n:]).all()), "a guard band was written"
    return view, check
