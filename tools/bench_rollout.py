"""Attention rollout of the ViViT at the metric shape (B = 8 clips of 32 x 3 x 224^2, d = 512, depth 4 + 4, 8 heads of 64:
256 space sequences of 197 tokens, 8 temporal sequences of 33, bf16) on the MI355X, timed with hipEvents (warm-up, then the
median over the timed iterations; callables of one group ALTERNATE in one timed loop).  One JSON line on stdout.

    timeout -k 10 600 python tools/bench_rollout.py [--warmup 3] [--steps 15] [--batch 8]

  forward          the eval() forward alone, under torch.no_grad()
  maps             AttentionRollout.maps(clip): that forward under the tap plus every rollout launch
  rollout_launches the rollout launches alone on that forward's own taps (per stack one start + L - 1 steps, then the
                   video launch); maps - forward should be this
  step_space       one dense ops.rollout_step on a space layer's q, k, lse [256, 8, 197, 64]
  attention_fwd    ops.attention_fwd on the same q, k (and v) in the same loop: a step does one of its two products and
                   writes N floats per sequence instead of N x 64, so it should not take longer (a report, not a gate)
  step_time        one dense step of the temporal stack [8, 8, 33, 64]
  start_space      the start of the space recurrence (rollout_from_probs on the folded layer's P, or the one-hot step)
  video            ops.rollout_video
  eager            the textbook form with torch's eager operators on the same taps: materialised softmax(QK^T) per dense
                   layer, head mean, residual mix, bmm chain of N x N matrices, CLS row, time x space, scaling
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(min(16, torch.get_num_threads()))


def _stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(round(f * (len(s) - 1))))]  # noqa: E731
    return {"median_us": round(q(0.5) * 1e3, 2), "p10_us": round(q(0.1) * 1e3, 2), "p90_us": round(q(0.9) * 1e3, 2), "n": len(s)}


def _time(fns, warmup, steps):
    """Time the callables of ``fns`` alternately -> one list of milliseconds per callable."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(steps)]
    for row in ev:
        for fn, (a, b) in zip(fns, row):
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    return [[row[i][0].elapsed_time(row[i][1]) for row in ev] for i in range(len(fns))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=8)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rollout needs the MI355X: a timing on the CPU says nothing")
    from dvt_amd import functional as F, ops
    from dvt_amd.models.vit import ViViT
    from dvt_amd.rollout import AttentionRollout, _stack_row

    B, T, depth, heads, dh, rho = a.batch, 32, 4, 8, 64, 0.5
    torch.manual_seed(1130)
    net = ViViT(224, 16, 19, T, dim=512, depth=depth, heads=heads, dim_head=dh, compute_dtype=torch.bfloat16).cuda().eval()
    clip = torch.from_numpy(np.random.default_rng(7).standard_normal((B, T, 3, 224, 224)).astype(np.float32)).cuda()
    ro = AttentionRollout(net, residual=rho)
    res = {"batch": B, "frames": T, "warmup": a.warmup, "steps": a.steps, "dtype": "bf16"}

    def forward():
        with torch.no_grad():
            return net(clip)

    t_fwd, t_maps = _time([forward, lambda: ro.maps(clip)], a.warmup, a.steps)
    res["forward"], res["maps"] = _stats(t_fwd), _stats(t_maps)

    with torch.no_grad(), F.attention_tap() as taps:
        net(clip)
    space, time = taps[:depth], taps[depth:]
    res["taps"] = [t.kind for t in taps]
    d0 = space[0]
    S, H, N, _ = d0.q.shape
    res["space_step_plan"] = ops.rollout_plan(d0.q, d0.k, torch.empty((S, N), device="cuda"))._asdict()

    def launches():
        return ops.rollout_video(_stack_row(space, rho), _stack_row(time, rho))

    r_mid = _stack_row(space[1:], rho)
    v = d0.packed.view(S, N, 3, H, dh)[:, :, 2].permute(0, 2, 1, 3)
    o = torch.empty((S, N, H, dh), dtype=d0.q.dtype, device="cuda").permute(0, 2, 1, 3)
    lse_buf = torch.empty_like(d0.lse)
    t0 = time[0]
    r_t = _stack_row(time[1:], rho)
    r_space, r_time = _stack_row(space, rho), _stack_row(time, rho)

    def eager_stack(layers, n_tok):
        R = None
        start = None
        for tp in layers:
            if tp.kind == "folded":                        # the CLS row of the last layer is all the model computed
                start = rho * torch.nn.functional.one_hot(torch.zeros(tp.P.shape[0], dtype=torch.long, device="cuda"), n_tok) \
                    + (1 - rho) * tp.P[:, :, :tp.heads].mean(2)
                continue
            p = torch.softmax(torch.matmul(tp.q.float(), tp.k.float().transpose(2, 3)) * tp.dh ** -0.5, dim=-1).mean(1)
            if p.shape[1] == 1:                            # a single-query layer: its row is the start vector
                start = (1 - rho) * p[:, 0]
                start[:, 0] += rho
                continue
            Ah = rho * torch.eye(n_tok, device="cuda") + (1 - rho) * p
            R = Ah if R is None else torch.bmm(Ah, R)
        return torch.bmm(start[:, None, :], R)[:, 0] if start is not None else R[:, 0]

    def eager():
        rs, rt = eager_stack(space, N), eager_stack(time, T + 1)
        vid = rt[:, 1:, None] * rs.view(B, T, N)[:, :, 1:]
        flat = vid.reshape(B, -1)
        r = flat - flat.amin(1, keepdim=True)
        return vid, (r / (1e-7 + r.amax(1, keepdim=True))).view(vid.shape)

    groups = {
        "rollout_launches": launches,
        "eager": eager,
        "step_space": lambda: ops.rollout_step(d0.q, d0.k, d0.lse, r_mid, residual=rho),
        "attention_fwd": lambda: ops.attention_fwd(d0.q, d0.k, v, o, dh ** -0.5, lse=lse_buf),
        "step_time": lambda: ops.rollout_step(t0.q, t0.k, t0.lse, r_t, residual=rho),
        "start_space": lambda: _stack_row(space[-1:], rho),
        "video": lambda: ops.rollout_video(r_space, r_time),
    }
    for name, ms in zip(groups, _time(list(groups.values()), a.warmup, a.steps)):
        res[name] = _stats(ms)
    raw, _ = launches()
    res["max_rel_vs_eager"] = float((raw - eager()[0]).abs().max() / eager()[0].abs().max())
    res["maps_minus_forward_us"] = round(res["maps"]["median_us"] - res["forward"]["median_us"], 2)
    res["step_over_attention_fwd"] = round(res["step_space"]["median_us"] / res["attention_fwd"]["median_us"], 3)
    res["eager_over_launches"] = round(res["eager"]["median_us"] / res["rollout_launches"]["median_us"], 2)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
