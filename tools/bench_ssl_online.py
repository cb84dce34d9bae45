"""The online probe step (SSLOnlineEval.on_train_batch_end's SSLEvaluator step) on the MI355X, timed with hipEvents:
the fused three-launch step against torch's eager ``nn.Sequential`` + ``BCELoss`` + ``torch.optim.SGD`` of the same modules
(a child process of its own), and the contrastive training step with and without the callback.  One JSON line on stdout.

    python tools/bench_ssl_online.py [--warmup 20] [--steps 100] [--dtypes f32,bf16] [--no-yardstick] [--probe-only]

Shape: B = 256 rows of the 305-wide projection (the reference's projection_size), hidden 512, 15 classes, dropout 0.1.
The launch count per step comes from running ``--probe-only --no-yardstick`` under ``rocprofv3 --kernel-trace --stats``.
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

B, D, H, C, P, LR = 256, 305, 512, 15, 0.1, 0.005
DTYPES = {"f32": torch.float32, "bf16": torch.bfloat16}
CT = dict(input_shape=4608, hidden_layer=2048, projection_size=D, output_shape=128, batch_size=B, num_samples=50000,
          aggregation="concat", learning_rate=5e-6, weight_decay=0.09, epochs=500)


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


def _data(dtype):
    g = torch.Generator().manual_seed(0)
    return torch.randn(B, D, generator=g).to(dtype).cuda(), (torch.rand(B, C, generator=g) < 0.2).float().cuda()


def bench_probe(dtype, warmup, steps):
    from dvt_amd.models.evaluator import SSLEvaluator
    torch.manual_seed(0)
    e = SSLEvaluator(D, C, n_hidden=H, p=P).cuda().train()
    e.compute_dtype = dtype
    x, y = _data(dtype)
    return {"eager": _stats(_time(lambda: e.step(x, y, LR), warmup, steps))}


def bench_contrastive(dtype, warmup, steps):
    from dvt_amd import dp, metrics
    from dvt_amd import functional as F
    from dvt_amd.models.contrastivemodel import SpatioTemporalContrastiveModel
    torch.manual_seed(0)
    m = SpatioTemporalContrastiveModel(dict(CT)).cuda().train()
    m.compute_dtype = dtype
    flat = dp.FlatParameters(m, compute_dtype=None if dtype == torch.float32 else dtype)
    (opt,), (sched,) = m.configure_optimizers()
    sched.step()
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2 * B, CT["input_shape"], generator=g).to(dtype).cuda()
    y = (torch.rand(B, C, generator=g) < 0.2).float().cuda()
    cb = metrics.SSLOnlineEval(drop_p=P, z_dim=D, num_classes=C)
    cb.on_pretrain_routine_start(None, m)

    def step():
        flat.zero_grad()
        _, out = m._run(x, 2)
        loss = m._loss_rows(F.l2_normalize(out))
        loss.backward()
        flat.finish_backward()
        flat.adam_step(opt.lr_dev(0), weight_decay=CT["weight_decay"])

    def step_cb():                                        # + what on_train_batch_end adds: the embedding forward, the probe step
        step()
        with torch.no_grad():
            emb, _ = m(x[:B])
        m.non_linear_evaluator.step(emb, y, cb.lr)

    return {"step": _stats(_time(step, warmup, steps)), "step_with_callback": _stats(_time(step_cb, warmup, steps))}


def bench_torch(dtype, warmup, steps):
    torch.manual_seed(0)
    net = nn.Sequential(nn.Flatten(), nn.Dropout(P), nn.Linear(D, H, bias=False), nn.BatchNorm1d(H), nn.ReLU(inplace=True),
                        nn.Dropout(P), nn.Linear(H, C)).cuda().to(dtype)
    opt = torch.optim.SGD(net.parameters(), lr=LR)
    loss_fn = nn.BCELoss()
    x, y = _data(dtype)

    def step():                                           # as the reference's callback: no zero_grad
        loss = loss_fn(torch.sigmoid(net(x).float()), y)
        loss.backward()
        opt.step()

    return {"eager": _stats(_time(step, warmup, steps))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--dtypes", default="f32,bf16")
    ap.add_argument("--no-yardstick", action="store_true")
    ap.add_argument("--probe-only", action="store_true")
    ap.add_argument("--torch-child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    names = a.dtypes.split(",")
    if a.torch_child:
        print(json.dumps({n: bench_torch(DTYPES[n], a.warmup, a.steps) for n in names}))
        return
    res = {"shape": dict(B=B, D=D, H=H, C=C, p=P), "probe": {n: bench_probe(DTYPES[n], a.warmup, a.steps) for n in names}}
    if not a.probe_only:
        res["contrastive"] = {n: bench_contrastive(DTYPES[n], a.warmup, a.steps) for n in names}
    if not a.no_yardstick:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child", "--warmup", str(a.warmup),
                            "--steps", str(a.steps), "--dtypes", a.dtypes], capture_output=True, text=True, timeout=600)
        res["torch"] = (json.loads(p.stdout.strip().splitlines()[-1]) if p.returncode == 0
                        else {"error": f"exit {p.returncode}", "stderr": p.stderr[-2000:]})
    print(json.dumps(res))


if __name__ == "__main__":
    main()
