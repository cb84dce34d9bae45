"""Global-norm gradient clipping and gradient accumulation on the MI355X, timed with hipEvents (warm-up, then the median
over the timed iterations).  One JSON line on stdout.

    python tools/bench_accumulate.py [--warmup 10] [--steps 50] [--windows 12] [--skip-step]

Clipping, at the parameter sets of the ViViT metric model (bench.py: d = 512, depth 4, 28.8 M parameters) and of
SpatioTemporalContrastiveModel (tools/bench_lars.py: 14.4 M), random gradients, compared on the same GPU:
  clip_flat      FlatParameters.clip_grad_norm_: two launches (partials; scale) over one segment, the clip active (the
                 threshold drops 10 % per call, so every call scales)
  clip_flat_idle the same with a threshold nothing reaches: the coefficient clamps to 1 and the scale pass writes nothing
  norm_flat      ops.grad_norm alone: two launches (partials; total)
  clip_optim     optim.clip_grad_norm_ over the separate gradient tensors (one segment per tensor), the clip active
  torch          torch.nn.utils.clip_grad_norm_ on the same separate tensors
  floor          12 bytes per element / HBM peak (bench.py's HBM_PEAK_GBS): one read for the norm, a read and a write for
                 the scale, every pass counted from HBM
Accumulation (unless --skip-step): the reference-default FrameTransformer(model="vid") at batch 2, a window of k = 4:
  micro_no_sync  forward + backward + finish_backward of a non-final micro-batch inside no_sync()
  micro_final    the same for the final micro-batch (buckets counted, unwritten slices settled)
  update         clip_grad_norm_(1.0) + adamw_step
  plain_step     zero_grad + forward + backward + finish_backward + adamw_step, the step without accumulation
All eager launches at world 1 without a communicator: host-side launch cost is part of every figure.
"""
from __future__ import annotations

import argparse
import contextlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0
K = 4


def _stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(round(f * (len(s) - 1))))]  # noqa: E731
    return {"median_us": round(q(0.5) * 1e3, 2), "p10_us": round(q(0.1) * 1e3, 2), "p90_us": round(q(0.9) * 1e3, 2), "n": len(s)}


def _time(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
    for a, b in ev:
        a.record()
        fn()
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) for a, b in ev]


def _vivit():
    from dvt_amd.models.vit import ViViT
    torch.manual_seed(1130)
    return ViViT(224, 16, 19, 32, dim=512, depth=4, heads=8, dim_head=64, compute_dtype=torch.bfloat16).cuda().train()


def _contrastive():
    from dvt_amd.models.contrastivemodel import SpatioTemporalContrastiveModel
    torch.manual_seed(0)
    cfg = dict(input_shape=4608, hidden_layer=2048, projection_size=305, output_shape=128, batch_size=256,
               num_samples=50000, aggregation="concat", learning_rate=0.3, weight_decay=1.5e-6, epochs=500,
               optimizer="lars", momentum=0.9)
    return SpatioTemporalContrastiveModel(cfg).cuda().train()


def _clip_figures(make, a):
    from dvt_amd import dp, ops, optim
    gen = torch.Generator().manual_seed(1)
    flat = dp.FlatParameters(make(), compute_dtype=None)
    for p in flat.params:
        p.grad.copy_(torch.randn(p.shape, generator=gen) * 0.02)
    n = sum(p.numel() for p in flat.params)
    res = {"elements": n, "flat_elements": flat.total, "tensors": len(flat.params)}
    flat.clip_grad_norm_(1.0)
    res["plan_blocks"] = flat._clip_table.plan.blocks
    bound = [1.0]

    def shrinking(clip):
        """A threshold 10 % lower at every call: the coefficient stays near 0.9, so every call scales (a fixed threshold
        is reached after two calls, and the scale pass of every later one writes nothing)."""
        def call():
            bound[0] *= 0.9
            clip(bound[0])
        return call

    res["clip_flat"] = _stats(_time(shrinking(lambda m: flat.clip_grad_norm_(m)), a.warmup, a.steps))
    res["clip_flat_idle"] = _stats(_time(lambda: flat.clip_grad_norm_(1e30), a.warmup, a.steps))
    res["norm_flat"] = _stats(_time(lambda: ops.grad_norm(flat._clip_table), a.warmup, a.steps))
    params = [torch.nn.Parameter(torch.empty(p.shape, device="cuda")) for p in flat.params]
    for p in params:
        p.grad = torch.randn(p.shape, generator=gen).cuda() * 0.02
    bound[0] = 1.0
    res["clip_optim"] = _stats(_time(shrinking(lambda m: optim.clip_grad_norm_(params, m)), a.warmup, a.steps))
    res["torch"] = _stats(_time(shrinking(lambda m: torch.nn.utils.clip_grad_norm_(params, m)), a.warmup, a.steps))
    res["floor"] = {"bytes": flat.total * 12, "us": round(flat.total * 12 / (HBM_PEAK_GBS * 1e9) * 1e6, 2)}
    return res


def _step_figures(a):
    from dvt_amd.dp import FlatParameters
    from dvt_amd.models.frame_transformer import FrameTransformer
    torch.manual_seed(1130)
    B = 2                                                          # config.yaml:2
    net = FrameTransformer(batch_size=B, seq_len=13, cls=1, model="vid", opt="adamW", learning_rate=5e-6,
                           weight_decay=0.09, momentum=0.005).cuda().train()
    flat = FlatParameters(net, compute_dtype=torch.bfloat16)
    flat.sync_compute_copy()
    gen = torch.Generator().manual_seed(1130)
    xs = [torch.randn(B, 13, 12, 3, 112, 112, generator=gen).cuda() for _ in range(K)]
    y = (torch.rand(B, 19, generator=gen) < 0.2).float().cuda()
    one = torch.full((), flat.loss_scale, device="cuda")
    part = torch.full((), flat.accumulation_scale(K), device="cuda")

    def plain():
        flat.zero_grad()
        net.training_step((y, None, xs[0]), 0).backward(one)
        flat.finish_backward()
        flat.adamw_step(lr=5e-6, weight_decay=0.09)

    res = {"k": K, "batch": B, "plain_step": _stats(_time(plain, 3, a.windows))}
    marks = {"micro_no_sync": [], "micro_final": [], "update": []}

    def timed(key, fn):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        marks[key].append((e0, e1))

    def micro(j):
        net.training_step((y, None, xs[j]), 0).backward(part)
        flat.finish_backward()

    def update():
        flat.clip_grad_norm_(1.0)
        flat.adamw_step(lr=5e-6, weight_decay=0.09)

    for w in range(3 + a.windows):
        if w == 3:
            torch.cuda.synchronize()
            for v in marks.values():
                v.clear()
        flat.zero_grad()
        for j in range(K):
            with (flat.no_sync() if j < K - 1 else contextlib.nullcontext()):
                timed("micro_no_sync" if j < K - 1 else "micro_final", lambda: micro(j))
        timed("update", update)
    torch.cuda.synchronize()
    for key, evs in marks.items():
        res[key] = _stats([e0.elapsed_time(e1) for e0, e1 in evs])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=12)
    ap.add_argument("--skip-step", action="store_true")
    a = ap.parse_args()
    res = {"warmup": a.warmup, "steps": a.steps, "hbm_peak_gbs": HBM_PEAK_GBS}
    res["vivit"] = _clip_figures(_vivit, a)
    res["contrastive"] = _clip_figures(_contrastive, a)
    if not a.skip_step:
        res["frametransformer"] = _step_figures(a)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
