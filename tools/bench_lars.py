"""The LARS step at SpatioTemporalContrastiveModel's parameter set on the MI355X, timed with hipEvents (warm-up, then the
median over the timed iterations).  One JSON line on stdout.

    python tools/bench_lars.py [--warmup 10] [--steps 50]

Shape as tools/bench_contrastive.py: input 4608, hidden 2048, projection 305 and (chosen there; the reference pins only
the projection) output 128 -- ten tensors from 4608 x 2048 down to the two 305-element projection biases and the
128-element output bias, 14.4 M parameters.  Compared on the same GPU:
  lars_flat    FlatParameters.lars_step (two launches: norms, update + bf16 mirror), momentum 0.9, the two weight decays of
               exclude_from_wt_decay
  lars_optim   optim.LARS.step on separate tensors (two groups: four launches, no mirror), gradients written in place
  lars_optim_fresh  the same with other gradient tensors every step, as after torch's zero_grad(set_to_none=True): plus
               one copy of each group's table rows
  sumsq        dvt_lars_sumsq alone (the norms launch plus the per-segment reduce)
  torch_eager  the rule restated with torch operators per parameter, as pl_bolts runs it (its norm tests synchronise)
  adam_flat    FlatParameters.adam_step on the same buffers: the one-launch streaming baseline
  floor        bytes moved / HBM peak (bench.py's HBM_PEAK_GBS): every pass counted from HBM -- norms read p, g; the update
               reads p, g, buf and writes p, buf and the 16-bit mirror = 30 bytes per element
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

D, HID, PROJ, OUT = 4608, 2048, 305, 128
CFG = dict(input_shape=D, hidden_layer=HID, projection_size=PROJ, output_shape=OUT, batch_size=256, num_samples=50000,
           aggregation="concat", learning_rate=0.3, weight_decay=1.5e-6, epochs=500, optimizer="lars", momentum=0.9)
HBM_PEAK_GBS = 8000.0
TRUST = 0.0001


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


def _model():
    from dvt_amd.models.contrastivemodel import SpatioTemporalContrastiveModel
    torch.manual_seed(0)
    return SpatioTemporalContrastiveModel(dict(CFG)).cuda().train()


@torch.no_grad()
def _torch_lars(params, grads, bufs, wds, lr, momentum):
    for p, g, buf, wd in zip(params, grads, bufs, wds):
        d = g
        pn, gn = torch.norm(p), torch.norm(g)
        if wd != 0 and pn != 0 and gn != 0:
            d = (g + wd * p) * (TRUST * pn / (gn + wd * pn + 1e-8))
        buf.mul_(momentum).add_(d)
        p.add_(buf, alpha=-lr)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    from dvt_amd import dp, ops

    gen = torch.Generator().manual_seed(1)
    res = {"shape": dict(D=D, hidden=HID, proj=PROJ, out=OUT), "warmup": a.warmup, "steps": a.steps}

    m = _model()
    flat = dp.FlatParameters(m, compute_dtype=torch.bfloat16)
    flat.sync_compute_copy()
    for p in flat.params:
        p.grad.copy_(torch.randn(p.shape, generator=gen) * 0.02)
    wds = [0.0 if "bias" in k else CFG["weight_decay"] for k, _ in m.named_parameters()]
    n = sum(p.numel() for p in flat.params)
    lr = torch.full((1,), CFG["learning_rate"], dtype=torch.float32, device="cuda")
    res["elements"], res["tensors"] = n, len(flat.params)
    res["lars_flat"] = _stats(_time(lambda: flat.lars_step(lr, momentum=0.9, weight_decay=wds, trust_coefficient=TRUST),
                                    a.warmup, a.steps))
    res["sumsq"] = _stats(_time(lambda: ops.lars_sumsq(flat._lars_table), a.warmup, a.steps))
    res["plan"] = flat._lars_table.plan._asdict() | {"chunk_begin": None}
    res["adam_flat"] = _stats(_time(lambda: flat.adam_step(lr, weight_decay=CFG["weight_decay"]), a.warmup, a.steps))

    m2 = _model()
    (opt,), _ = m2.configure_optimizers()
    opt.param_groups[0]["lr"] = opt.param_groups[1]["lr"] = CFG["learning_rate"]
    for p in m2.parameters():
        p.grad = torch.randn(p.shape, generator=gen).cuda() * 0.02
    res["lars_optim"] = _stats(_time(opt.step, a.warmup, a.steps))
    sets = [[p.grad for p in m2.parameters()], [p.grad.clone() for p in m2.parameters()]]
    turn = [0]

    def fresh():
        turn[0] ^= 1
        for p, g in zip(m2.parameters(), sets[turn[0]]):
            p.grad = g
        opt.step()
    res["lars_optim_fresh"] = _stats(_time(fresh, a.warmup, a.steps))

    m3 = _model()
    params = [p.data for p in m3.parameters()]
    grads = [torch.randn(p.shape, generator=gen).cuda() * 0.02 for p in params]
    bufs = [torch.zeros_like(p) for p in params]
    res["torch_eager"] = _stats(_time(lambda: _torch_lars(params, grads, bufs, wds, CFG["learning_rate"], 0.9),
                                      a.warmup, a.steps))

    for key, bytes_per_elem in (("floor_lars_flat", 30), ("floor_lars_optim", 28), ("floor_adam_flat", 30), ("floor_sumsq", 8)):
        res[key] = {"bytes": n * bytes_per_elem, "us": round(n * bytes_per_elem / (HBM_PEAK_GBS * 1e9) * 1e6, 2)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
