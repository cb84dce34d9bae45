"""Gradient accumulation (``FlatParameters.no_sync``) and the clipping surface, on the CPU.

As in test_dp_gloo.py the GPU kernels cannot run here: each rank takes the CPU oracle's gradients of its clips and hands them
to ``dp.FlatParameters`` through the GradSink protocol the HIP backward uses.  Two gloo ranks, two micro-batches of one clip
each, the first under ``no_sync()``: the flat gradient must be the single-process gradient of the four clips, and the
exchange must run once per window.
"""
import os

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests.test_dp_gloo import _data, _free_port, _model, _oracle_grads

TWICE = ("mlp_head.1.weight", "space_transformer.layers.0.1.fn.net.0.bias")   # written twice in the final pass
NEVER = "temporal_token"          # window 0: written in no pass
FIRST_ONLY = "space_token"        # written in the first pass of a window only (shares the last bucket with NEVER)
K = 2


def _write(sink, part):
    if sink.fresh:                    # the writer protocol of functional.py: buf / fresh, then mark_written
        sink.buf.copy_(part)
    else:
        sink.buf.add_(part)
    sink.mark_written()


def _worker(rank, world, port, bucket_mb, out):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    from dvt_amd.dp import FlatParameters
    net = _model()
    flat = FlatParameters(net, bucket_mb=bucket_mb, compute_dtype=None)
    flat.broadcast_parameters(0)
    named = dict(net.named_parameters())
    names = list(named)
    calls = {"in": 0, "out": 0}
    plain = flat._all_reduce

    def counted(t, via=None):
        calls["in" if flat._no_sync else "out"] += 1
        return plain(t, via)

    flat._all_reduce = counted
    x, y = _data()
    scale = flat.accumulation_scale(K)
    assert scale == 1.0 / (world * K) and flat.loss_scale == 1.0 / world
    grads = [_oracle_grads(net, x[c:c + 1], y[c:c + 1], scale) for c in (rank * K, rank * K + 1)]
    windows, counts, lates = [], [], []
    for w in range(2):                # second window: the sums of the first must be overwritten, the counts re-armed
        calls["in"] = calls["out"] = 0
        flat.zero_grad()
        with flat.no_sync():
            for k in reversed(names):                      # backward order
                if k == NEVER and w == 0:
                    continue
                _write(named[k]._dvt_sink, grads[0][k])
            assert not any(flat._launched) and not flat._handles
            flat.finish_backward()
            # the local part only: nothing zeroed, nothing marked unwritten, no skip mask from this pass
            assert not any(s.unwritten for s in flat.sinks) or w == 1
            assert flat.sinks[names.index(NEVER)]._fresh == (w == 0)
        assert calls == {"in": 0, "out": 0}
        for k in reversed(names):
            if (k == NEVER and w == 0) or k == FIRST_ONLY:
                continue
            s = named[k]._dvt_sink
            assert not s.fresh or (k == NEVER)             # every later write of the window accumulates
            _write(s, grads[1][k] * (0.25 if k in TWICE else 1.0))
        # FIRST_ONLY was not written in this pass: its bucket (the last one) has not left
        assert not flat._launched[named[FIRST_ONLY]._dvt_sink.bucket]
        for k in TWICE:
            _write(named[k]._dvt_sink, grads[1][k] * 0.75)
        lates.append(sum(s.late_written for s in flat.sinks))
        flat.finish_backward()
        i = names.index(NEVER)
        if w == 0:
            assert flat.sinks[i].unwritten and flat.skip_mask is not None
            assert int(flat.skip_mask.sum()) == (flat.params[i].numel() + 63) // 64
        else:
            assert flat.skip_mask is None and not any(s.unwritten for s in flat.sinks)
        windows.append(flat.grad.clone())
        counts.append(dict(calls))
    if rank == 0:
        torch.save({"windows": windows, "counts": counts, "lates": lates, "nb": len(flat.bucket_ranges), "names": names,
                    "offsets": flat.offsets}, out)
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("bucket_mb", [32.0, 0.05])
def test_two_ranks_two_micro_batches_equal_the_four_clip_gradient(tmp_path, bucket_mb):
    """Fails on a tree without ``no_sync``.  Per window: no collective inside ``no_sync``, one per bucket plus one per late
    side buffer outside; a parameter written twice in the final pass (late with small buckets), one written in no pass
    (window 0), one written in the first pass only (its bucket leaves at finish_backward)."""
    import dvt_amd  # noqa: F401  (registers the package alias before spawn pickles the worker)
    out = str(tmp_path / "r0.pt")
    mp.spawn(_worker, args=(2, _free_port(), bucket_mb, out), nprocs=2, join=True)
    res = torch.load(out)
    net = _model()
    x, y = _data()
    ref = _oracle_grads(net, x, y, 1.0)                     # single process, the four clips as one batch
    clip = [_oracle_grads(net, x[c:c + 1], y[c:c + 1], 0.25) for c in range(4)]
    params = dict(net.named_parameters())
    nb = res["nb"]
    assert nb == (1 if bucket_mb > 1 else 7)
    for w in range(2):
        n_late = res["lates"][w]
        assert n_late == (0 if bucket_mb > 1 else len(TWICE))
        assert res["counts"][w] == {"in": 0, "out": nb + n_late}, (w, res["counts"][w])
        for k, off in zip(res["names"], res["offsets"]):
            n = params[k].numel()
            got = res["windows"][w][off:off + n].view(params[k].shape)
            if k == NEVER and w == 0:
                want = torch.zeros_like(ref[k])
            elif k == FIRST_ONLY:
                want = clip[0][k] + clip[2][k]              # the first micro-batch of either rank
            else:
                want = ref[k]
            assert torch.allclose(got, want, rtol=1e-4, atol=1e-6), (w, k)


def _expected_pending(flat):
    """Independent restatement of zero_grad's rule: a bucket waits for each of its sinks except those nobody wrote in the
    previous step and whose slice still holds finish_backward's zeros; a bucket left with none waits for finish_backward."""
    want = [0] * len(flat.bucket_ranges)
    for s in flat.sinks:
        if not (s.unwritten and s._zeroed):
            want[s.bucket] += 1
    return [n if n > 0 else 1 << 30 for n in want]


def test_window_without_no_sync_keeps_every_flag_and_count():
    """World 1, no ``no_sync()``: the write sequence of a plain step -- one parameter dead, one written twice -- leaves
    ``unwritten``, ``skip_mask``, ``_pending`` and ``_launched`` as the plain step always did."""
    from dvt_amd.dp import FlatParameters
    net = _model()
    flat = FlatParameters(net, bucket_mb=0.05, compute_dtype=None)
    named = dict(net.named_parameters())
    names = list(named)
    i_never = names.index(NEVER)
    for step in range(3):
        want = _expected_pending(flat)
        flat.zero_grad()
        assert flat._pending == want and flat._pass == 0 and not flat._no_sync
        if step == 0:
            assert want == flat.bucket_size
        else:                                               # the dead parameter's bucket no longer waits for it
            b = flat.sinks[i_never].bucket
            assert want[b] == flat.bucket_size[b] - 1 and flat.sinks[i_never]._uncounted
        for k in reversed(names):
            if k == NEVER:
                continue
            s = named[k]._dvt_sink
            before = list(flat._pending)
            assert s.fresh
            s.buf.fill_(1.0)
            s.mark_written()
            assert flat._pending[s.bucket] == before[s.bucket] - 1
            assert flat._launched[s.bucket] == (flat._pending[s.bucket] == 0)
            assert not s.fresh
            before = list(flat._pending)
            s.buf.add_(1.0)                                 # a second write of the same pass counts nothing
            s.mark_written()
            assert flat._pending == before and not s.late_written
        b = flat.sinks[i_never].bucket
        assert flat._launched == [i != b or step > 0 for i in range(len(flat.bucket_ranges))]
        flat.finish_backward()
        assert all(flat._launched) and flat._pass == 0
        assert [s.index for s in flat.sinks if s.unwritten] == [i_never] and flat._skip_sig == (i_never,)
        assert int(flat.skip_mask.sum()) == 1 and int(flat.skip_mask[flat.offsets[i_never] // 64]) == 1
        assert float(named[NEVER].grad.abs().max()) == 0.0 and float(named["space_token"].grad.min()) == 2.0


def test_accumulation_at_world_one_counts_per_pass():
    """The per-pass counts without any exchange: k = 3, the buckets are 'launched' (flagged) in the final pass only, each
    when its last sink is written in that pass; the sums are those of three writes."""
    from dvt_amd.dp import FlatParameters
    net = _model()
    flat = FlatParameters(net, bucket_mb=0.05, compute_dtype=None)
    named = dict(net.named_parameters())
    names = list(named)
    flat.zero_grad()
    for j in range(3):
        with (flat.no_sync() if j < 2 else __import__("contextlib").nullcontext()):
            for k in reversed(names):
                s = named[k]._dvt_sink
                assert s.fresh == (j == 0)
                if s.fresh:
                    s.buf.fill_(float(j + 1))
                else:
                    s.buf.add_(float(j + 1))
                s.mark_written()
                assert flat._launched[s.bucket] == (j == 2 and flat._pending[s.bucket] == 0)
            if j < 2:
                assert not any(flat._launched)
            flat.finish_backward()
            assert flat._pass == min(j + 1, 2)
    assert all(flat._launched) and flat.skip_mask is None
    for k, p in named.items():
        assert float(p.grad.min()) == 6.0 and float(p.grad.max()) == 6.0, k
    with pytest.raises(RuntimeError, match="nest"):
        with flat.no_sync():
            with flat.no_sync():
                pass
    assert not flat._no_sync


def test_surface_of_accumulation_and_clipping():
    import inspect
    from dvt_amd import _lib as L, dp, graph, ops, optim
    assert L.ABI_VERSION == 5
    for name in ("dvt_grad_norm", "dvt_grad_clip"):
        assert name in L.SIGNATURES, name
    assert L.ENUMS["dvt_norm_kind"] == {"DVT_NORM_2": 0, "DVT_NORM_INF": 1}
    for owner, name in ((ops, "grad_norm"), (ops, "grad_clip_"), (dp.FlatParameters, "no_sync"),
                        (dp.FlatParameters, "accumulation_scale"), (dp.FlatParameters, "clip_grad_norm_"),
                        (optim, "clip_grad_norm_"), (graph, "capture_accumulated_step")):
        assert callable(getattr(owner, name)), name
    assert list(inspect.signature(optim.clip_grad_norm_).parameters) == ["parameters", "max_norm", "norm_type",
                                                                         "error_if_nonfinite"]
    assert list(inspect.signature(graph.capture_accumulated_step).parameters) == ["micro_fn", "update_fn", "flat", "k",
                                                                                  "warmup"]
    assert "accumulate" in inspect.signature(dp.FlatParameters.enable_loss_scaling).parameters
    assert ops.norm_kind(2) == 0 and ops.norm_kind(2.0) == 0 and ops.norm_kind(float("inf")) == 1
    net = _model()
    flat = dp.FlatParameters(net, compute_dtype=None)
    assert flat.accumulation_scale(4) == 0.25 and flat.loss_scale == 1.0
    for bad in (3, 1, 0.5, "fro"):
        with pytest.raises(NotImplementedError):
            flat.clip_grad_norm_(1.0, norm_type=bad)
        with pytest.raises(NotImplementedError):
            optim.clip_grad_norm_(net.parameters(), 1.0, norm_type=bad)
    with pytest.raises(NotImplementedError):
        optim.clip_grad_norm_(net.parameters(), 1.0, error_if_nonfinite=True)
