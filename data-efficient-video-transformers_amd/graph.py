"""hipGraph capture of a whole training step.

The step of the clip path is a fixed sequence of ~300 kernel launches, a third of
them microsecond-sized (the 33-token temporal encoder); launched one by one from
Python the host cannot keep the GPU fed.  ``capture_step`` records the sequence
once (HIP stream capture through ``torch.cuda.CUDAGraph``: every launch of
libdvt_hip.so on the capturing stream is recorded) and replays it with a single
``hipGraphLaunch`` per step.  Requirements on ``step_fn``: static shapes, inputs
read from fixed tensors, no host synchronisation (no ``.item()``), optimizer state
on the device (``dp.FlatParameters.adamw_step`` keeps its step counter there).

Data parallel: the gradient buckets' RCCL all-reduces (``dp.Communicator``: ``dvt_comm_allreduce``
on a side stream, forked from and joined to the compute stream through events) are
recorded in the same graph, so the N-GPU step is the same single ``hipGraphLaunch`` as
the one-GPU step.  ``capture_step_segments`` is the form for an exchange that cannot
be captured (gloo on the CPU rehearsal, or an RCCL build that refuses capture): the
step is cut at the exchange into two graphs with the collective launched between them.
"""
from __future__ import annotations

import contextlib
from typing import Callable, Tuple

import torch


def capture_step(step_fn: Callable[[], torch.Tensor], warmup: int = 3, flat=None) -> Tuple[Callable[[], None], torch.Tensor]:
    """Returns (replay, static_output).  ``replay()`` re-runs the captured step;
    ``static_output`` is the tensor returned by ``step_fn`` during capture (its
    storage is overwritten by every replay).  ``flat`` (a ``dp.FlatParameters``): its cached packed convolution
    weights are marked stale before the capture, so the one repack launch per step is recorded in the graph even when
    ``step_fn`` does not contain the optimizer step that normally invalidates them."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(max(1, warmup)):     # allocates workspaces, sets kernel attributes
            step_fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    if flat is not None:
        flat.invalidate_packed()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        out = step_fn()
    return graph.replay, out


def capture_step_segments(fwd_bwd_fn: Callable[[], torch.Tensor], exchange_fn: Callable[[], None],
                          update_fn: Callable[[], None], warmup: int = 3, flat=None) -> Tuple[Callable[[], None], torch.Tensor]:
    """Two graphs around an eagerly launched exchange:  replay() = graph(fwd_bwd) ; exchange_fn() ; graph(update).
    ``fwd_bwd_fn`` must leave the gradient exchange to ``exchange_fn`` (``FlatParameters.finish_backward(exchange=False)``
    then ``FlatParameters.exchange_all()``)."""
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(max(1, warmup)):
            fwd_bwd_fn()
            exchange_fn()
            update_fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    if flat is not None:
        flat.invalidate_packed()
    g1, g2 = torch.cuda.CUDAGraph(), torch.cuda.CUDAGraph()
    with torch.cuda.graph(g1):
        out = fwd_bwd_fn()
    exchange_fn()
    with torch.cuda.graph(g2, pool=g1.pool()):
        update_fn()

    def replay():
        g1.replay()
        exchange_fn()
        g2.replay()

    return replay, out


def capture_accumulated_step(micro_fn: Callable[[], torch.Tensor], update_fn: Callable[[], None], flat, k: int,
                             warmup: int = 3) -> Tuple[Callable[[int], None], torch.Tensor]:
    """A step made of ``k`` backward passes (``dp.FlatParameters.no_sync``).  Whether a writer overwrites or accumulates is
    a host flag frozen at capture, so one graph cannot serve every micro-batch; at most three, from one memory pool, do:

        first    zero_grad, micro_fn inside no_sync           (every first write overwrites; only when k > 1)
        middle   micro_fn inside no_sync                      (every write accumulates; only when k > 2)
        last     micro_fn outside no_sync -- with the bucket exchanges -- then update_fn

    ``micro_fn()``: forward, backward and ``flat.finish_backward()`` on static inputs, WITHOUT ``zero_grad`` (the helper
    opens the window); it returns the tensor to hand back (the loss).  ``update_fn()``: the optional
    ``flat.clip_grad_norm_`` and the optimizer step.  Returns (replay, static_output): ``replay(j)`` runs micro-batch
    ``j`` of a window (0 .. k - 1, in that order; the caller refreshes the static inputs between replays) and
    ``static_output`` is what ``micro_fn`` returned in the LAST graph, overwritten by every replay of it.

    As with ``capture_step``, the ``warmup`` windows run for real and advance weights, optimizer state and the loss
    scale; the captured window is recorded, not run, but host-side counters (``flat.step_count``) advance with it too.
    The set of parameters without a gradient must be the same in the warm-up and the captured windows
    (``FlatParameters`` raises its RuntimeError otherwise).

    Where the exchange cannot be captured (``flat.defer_exchange``: gloo, or an RCCL build that refuses capture) the
    last graph is cut as ``capture_step_segments`` cuts its step: graph(micro_fn, whose finish_backward then does the
    local part only), ``flat.exchange_all()`` launched eagerly, graph(update_fn)."""
    k = int(k)
    if k < 1:
        raise ValueError("capture_accumulated_step: k must be >= 1")
    cut = bool(flat.defer_exchange)

    def first():
        flat.zero_grad()
        with flat.no_sync():
            return micro_fn()

    def middle():
        with flat.no_sync():
            return micro_fn()

    def last_local():
        if k == 1:
            flat.zero_grad()
        with flat.exchange_outside() if cut else contextlib.nullcontext():
            return micro_fn()

    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        for _ in range(max(1, warmup)):     # allocates workspaces and tables, sets kernel attributes
            for j in range(k - 1):
                first() if j == 0 else middle()
            last_local()
            if cut:
                flat.exchange_all()
            update_fn()
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    flat.invalidate_packed()

    graphs = {}

    def capture(name, fn):
        g = torch.cuda.CUDAGraph()
        pool = next(iter(graphs.values())).pool() if graphs else None
        with torch.cuda.graph(g, pool=pool):
            out = fn()
        graphs[name] = g
        return out

    def last_whole():
        out = last_local()
        update_fn()
        return out

    if k > 1:
        capture("first", first)
    if k > 2:
        capture("middle", middle)
    if cut:
        out = capture("last", last_local)
        flat.exchange_all()
        capture("update", update_fn)
    else:
        out = capture("last", last_whole)

    def replay(j: int) -> None:
        if not 0 <= j < k:
            raise IndexError(f"micro-batch {j} of a window of {k}")
        if j == k - 1:
            graphs["last"].replay()
            if cut:
                flat.exchange_all()
                graphs["update"].replay()
        elif j == 0:
            graphs["first"].replay()
        else:
            graphs["middle"].replay()

    return replay, out
