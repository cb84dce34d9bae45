"""LSTMRegressor training step at the reference shape (src/main.py:40-42: B=64, T=200, F=4608, H=512, 4 layers) on the
MI355X: fwd + loss + bwd + Adam, timed with hipEvents, and the recurrent chain alone (µs per step, forward and
backward).  The yardstick, torch.nn.LSTM (MIOpen) + nn.Linear + nn.BCELoss + torch.optim.Adam on the same GPU, runs in a
child process of its own.  One JSON line on stdout.

    python tools/bench_lstm.py [--warmup 10] [--steps 50] [--dtypes f32,bf16] [--no-yardstick]

The kernel split (input-projection GEMMs against chain steps) comes from running this under
``rocprofv3 --kernel-trace --stats``.
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

B, T, FEAT, H, LAYERS = 64, 200, 4608, 512, 4
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


def _data(dtype):
    g = torch.Generator().manual_seed(0)
    x = torch.randn(B, T, FEAT, generator=g).to(dtype).cuda()
    y = (torch.rand(B, 15, generator=g) < 0.3).float().cuda()
    return x, y


def bench_ours(dtype, warmup, steps):
    import dvt_amd
    from dvt_amd import ops
    from dvt_amd.models.LSTM import LSTMRegressor
    torch.manual_seed(0)
    m = LSTMRegressor(n_features=FEAT, hidden_size=H, seq_len=T, batch_size=B, num_layers=LAYERS, dropout=0.2,
                      learning_rate=5e-5, criterion=nn.BCELoss()).cuda()
    m.compute_dtype = dtype
    opt = m.configure_optimizers()
    x, y = _data(dtype)

    def step():
        opt.zero_grad()
        m.loss(m(x), y).backward()
        opt.step()

    res = {"step": _stats(_time(step, warmup, steps))}
    # the chain alone, one layer: T launches forward, 1 + T backward
    whh = m.lstm.weight_hh_l1.detach().to(dtype).contiguous()
    G = torch.randn(B * T, 4 * H, device="cuda").to(dtype)
    out = {}

    def fwd():
        out["f"] = ops.lstm_seq_fwd(G, whh, None, None, B, T, want_last=True)

    fwd()
    _, _, gates, c, _ = out["f"]
    dh = torch.randn(B, T, H, device="cuda").to(dtype)
    f_ms = _stats(_time(fwd, 3, 20))["median_ms"]
    b_ms = _stats(_time(lambda: ops.lstm_seq_bwd(whh, gates, c, dh, None), 3, 20))["median_ms"]
    res["chain_fwd_us_per_step"] = 1e3 * f_ms / T
    res["chain_bwd_us_per_step"] = 1e3 * b_ms / T
    res["chain_ms_per_training_step"] = LAYERS * (f_ms + b_ms)
    return res


def bench_torch(dtype, warmup, steps):
    torch.manual_seed(0)
    lstm = nn.LSTM(FEAT, H, LAYERS, batch_first=True, dropout=0.2).cuda().to(dtype)
    lin = nn.Linear(H, 15).cuda().to(dtype)
    opt = torch.optim.Adam(list(lstm.parameters()) + list(lin.parameters()), lr=5e-5)
    x, y = _data(dtype)
    crit = nn.BCELoss()

    def step():
        opt.zero_grad()
        out, _ = lstm(x)
        crit(torch.sigmoid(lin(out[:, -1]).float()), y).backward()
        opt.step()

    return {"step": _stats(_time(step, warmup, steps))}


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
    res = {"shape": dict(B=B, T=T, F=FEAT, H=H, L=LAYERS), "ours": {n: bench_ours(DTYPES[n], a.warmup, a.steps) for n in names}}
    for n in names:
        r = res["ours"][n]
        r["us_per_recurrent_step"] = 1e3 * r["step"]["median_ms"] / (2 * LAYERS * T)
    if not a.no_yardstick:
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--torch-child", "--warmup", str(a.warmup),
                            "--steps", str(a.steps), "--dtypes", a.dtypes], capture_output=True, text=True, timeout=1200)
        if p.returncode == 0:
            res["torch_nn_lstm"] = json.loads(p.stdout.strip().splitlines()[-1])
            for n in names:
                res["torch_nn_lstm"][n]["us_per_recurrent_step"] = \
                    1e3 * res["torch_nn_lstm"][n]["step"]["median_ms"] / (2 * LAYERS * T)
        else:
            res["torch_nn_lstm"] = {"error": f"exit {p.returncode}", "stderr": p.stderr[-2000:]}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
