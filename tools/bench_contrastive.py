"""SpatioTemporalContrastiveModel training step on the MI355X: two views, fwd + L2-norm + ContrastiveLoss + bwd + Adam,
timed with hipEvents in three forms -- the product launched eagerly, the product as one captured hipGraph, and a torch
yardstick (nn modules + torch.optim.Adam, two forward passes as the reference runs them) in a child process of its own.
One JSON line on stdout.

    python tools/bench_contrastive.py [--warmup 10] [--steps 50] [--dtypes f32,bf16] [--no-yardstick]

Shape (chosen, not taken from the reference, which pins only projection_size = 305): B = 256 per view, D = 4608 (the
three-expert concatenation src/main.py:41 gives the LSTM: 2048 image + 2048 location + 512 video), hidden 2048,
projection 305, output 128.  The kernel split comes from running this under ``rocprofv3 --kernel-trace --stats``.
"""
from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
from torch import nn  # noqa: E402

B, D, HID, PROJ, OUT = 256, 4608, 2048, 305, 128
CFG = dict(input_shape=D, hidden_layer=HID, projection_size=PROJ, output_shape=OUT, batch_size=B, num_samples=50000,
           aggregation="concat", learning_rate=5e-6, weight_decay=0.09, epochs=500)
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}


def _stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(round(f * (len(s) - 1))))]  # noqa: E731
    return {"median_ms": q(0.5), "p10_ms": q(0.1), "p90_ms": q(0.9), "n": len(s)}


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


def _views():
    g = torch.Generator().manual_seed(0)
    return torch.randn(B, D, generator=g).cuda(), torch.randn(B, D, generator=g).cuda()


def bench_ours(dtype, warmup, steps):
    import dvt_amd
    from dvt_amd import dp, graph
    from dvt_amd import functional as F
    from dvt_amd.models.contrastivemodel import SpatioTemporalContrastiveModel
    torch.manual_seed(0)
    m = SpatioTemporalContrastiveModel(dict(CFG)).cuda().train()
    m.compute_dtype = dtype
    flat = dp.FlatParameters(m, compute_dtype=None if dtype == torch.float32 else dtype)
    (opt,), (sched,) = m.configure_optimizers()
    sched.step()                                         # epoch 1: a non-zero rate
    xi, xj = _views()
    x = torch.cat([xi, xj]).to(dtype)

    def step():
        flat.zero_grad()
        _, out = m._run(x, 2)
        loss = m._loss_rows(F.l2_normalize(out))
        loss.backward()
        flat.finish_backward()
        flat.adam_step(opt.lr_dev(0), weight_decay=CFG["weight_decay"])
        return loss

    eager = _stats(_time(step, warmup, steps))
    replay, _ = graph.capture_step(step, warmup=2)
    captured = _stats(_time(replay, warmup, steps))
    del dvt_amd
    return {"eager": eager, "captured": captured}


def bench_torch(dtype, warmup, steps):
    import torch.nn.functional as TF
    torch.manual_seed(0)
    enc = nn.Sequential(nn.Linear(D, HID, bias=False), nn.ReLU(inplace=True), nn.BatchNorm1d(HID),
                        nn.Linear(HID, HID, bias=False), nn.ReLU(inplace=True), nn.Linear(HID, PROJ)).cuda()
    proj = nn.Sequential(nn.ReLU(inplace=True), nn.Linear(PROJ, PROJ), nn.ReLU(inplace=True), nn.Dropout(0.1),
                         nn.Linear(PROJ, OUT)).cuda()
    params = list(enc.parameters()) + list(proj.parameters())
    opt = torch.optim.Adam(params, lr=5e-6, weight_decay=CFG["weight_decay"])
    xi, xj = _views()
    mask = (~torch.eye(2 * B, dtype=torch.bool, device="cuda")).float()

    def ntxent(a, b):
        reps = torch.cat([a, b])
        sim = TF.cosine_similarity(reps.unsqueeze(1), reps.unsqueeze(0), dim=2)
        pos = torch.cat([torch.diag(sim, B), torch.diag(sim, -B)])
        return torch.sum(-torch.log(torch.exp(pos / 0.5) / (mask * torch.exp(sim / 0.5)).sum(1))) / (2 * B)

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=dtype, enabled=dtype != torch.float32):
            oi = proj(enc(xi))
            oj = proj(enc(xj))
        loss = ntxent(TF.normalize(oi.float()), TF.normalize(oj.float()))
        loss.backward()
        opt.step()
        return loss

    return {"eager": _stats(_time(step, warmup, steps))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--torch-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    names = a.dtypes.split(",")
    if a.torch_child:
        print(json.dumps({n: bench_torch(DTYPES[n], a.warmup, a.steps) for n in names}))
        return
    flops = 2 * 3 * 2 * B * (D * HID + HID * HID + HID * PROJ + PROJ * PROJ + PROJ * OUT)
    res = {"shape": dict(B=B, D=D, hidden=HID, proj=PROJ, out=OUT), "gemm_gflop_per_step": flops / 1e9,
           "ours": {n: bench_ours(DTYPES[n], a.warmup, a.steps) for n in names}}
    if not a.no_yardstick:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child", "--warmup", str(a.warmup),
                            "--steps", str(a.steps), "--dtypes", a.dtypes], capture_output=True, text=True, timeout=900)
        if p.returncode == 0:
            res["torch"] = json.loads(p.stdout.strip().splitlines()[-1])
        else:
            res["torch"] = {"error": f"exit {p.returncode}", "stderr": p.stderr[-2000:]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
