"""The grouped AdamW step and the weight EMA at the metric ViViT's parameter set (bench.py: d = 512, depth 4, 28.8 M
elements, bf16 mirror) on the MI355X.  One process; every variant is warmed, then the variants alternate round by round;
a figure is the median over the rounds of the mean time of a window of back-to-back calls (device events), and the
spread of the rounds is reported beside it.  One JSON line on stdout.

    python tools/bench_optim_groups.py [--rounds 7] [--window 0.2] [--skip-step] [--skip-per-tensor]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_optim_groups.py --rounds 2 --skip-step --skip-per-tensor
    python tools/bench_optim_groups.py --kernel-trace DIR        # kernel times of that run, from its CSV

Variants (FlatParameters, random gradients, lr on the device):
  copy             ops.copy_ over the flat fp32 buffer: 8 B per element, the copy rate of this run
  adamw_step       the uniform one-launch step (adamw_fused_kernel): 30 B per element
  groups_1         adamw_groups_step with one group {1, wd}
  groups_2         ... with the two decay groups of optim.param_groups(layer_decay=None)
  groups_lrd       ... with the full layer-decay grouping at 0.75 (20 groups)
  groups_lrd_ema   the same with the weight EMA fused: 38 B per element
  ema_update       the EMA alone: 12 B per element
  lrd_plus_ema     groups_lrd followed by ema_update: what the fused launch replaces
  per_tensor       optim.AdamW.step on the same layer-decay groups over separate tensors (one launch per tensor, no mirror)
Captured step (unless --skip-step): zero_grad + ViViT.loss + backward + finish_backward + the optimizer step as one
hipGraph, b 8, T 32, 224^2, bf16, with adamw_step and with adamw_groups_step (layer decay 0.75, EMA off and on).
Floors: bytes per element x elements / 8 TB/s, and / the copy rate of the same run."""
from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0
LR, WD, LAYER_DECAY = 1e-4, 0.05, 0.75
BYTES = {"copy": 8, "adamw_step": 30, "groups_1": 30, "groups_2": 30, "groups_lrd": 30, "groups_lrd_ema": 38, "ema_update": 12,
         "lrd_plus_ema": 42}
KERNELS = ("adamw_fused_kernel", "adamw_groups_kernel", "ema_update_kernel", "adamw_kernel")


def _window(fn, seconds, calls):
    """Mean seconds per call over one window of back-to-back calls lasting at least ``seconds`` -> (mean, calls used)."""
    while True:
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        total = a.elapsed_time(b) * 1e-3
        if total >= seconds:
            return total / calls, calls
        calls = int(calls * max(2.0, 1.2 * seconds / max(total, 1e-6))) + 1


def _alternate(variants, rounds, seconds):
    """{name: fn} -> {name: [window mean per round]}; every variant warmed first, then round-robin."""
    hint = {}
    for name, fn in variants.items():
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        _, hint[name] = _window(fn, min(seconds, 0.05), 1)
    out = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            t, hint[name] = _window(fn, seconds, hint[name])
            out[name].append(t)
    torch.cuda.synchronize()
    return out


def _stats(ts):
    return {"median_us": round(statistics.median(ts) * 1e6, 2), "min_us": round(min(ts) * 1e6, 2),
            "max_us": round(max(ts) * 1e6, 2), "rounds": len(ts)}


def _vivit():
    from dvt_amd.models.vit import ViViT
    torch.manual_seed(1130)
    return ViViT(224, 16, 19, 32, dim=512, depth=4, heads=8, dim_head=64, compute_dtype=torch.bfloat16).cuda().train()


def bench_steps(a):
    from dvt_amd import dp, ops, optim
    gen = torch.Generator().manual_seed(1)
    net = _vivit()
    flat = dp.FlatParameters(net, compute_dtype=torch.bfloat16)
    flat.sync_compute_copy()
    for p in flat.params:
        p.grad.copy_(torch.randn(p.shape, generator=gen) * 0.02)
    lr_dev = torch.full((1,), LR, dtype=torch.float32, device="cuda")
    tables = {}
    for name, groups in (("groups_1", [{"params": flat.params, "weight_decay": WD}]),
                         ("groups_2", optim.param_groups(net, LR, WD)),
                         ("groups_lrd", optim.param_groups(net, LR, WD, layer_decay=LAYER_DECAY))):
        flat.set_param_groups(groups)
        tables[name] = (flat._group_table, flat.group_hyper, len(groups))
    ema = flat.enable_ema(0.9999)
    scratch = torch.empty_like(flat.data)

    def grouped(name, with_ema):
        def fn():
            flat._group_table, flat.group_hyper, _ = tables[name]
            flat.ema = ema if with_ema else None
            flat.adamw_groups_step(lr_dev)
        return fn

    def lrd_plus_ema():
        grouped("groups_lrd", False)()
        flat.ema = ema
        flat.ema_update()

    def ema_alone():
        flat.ema = ema
        flat.ema_update()

    variants = {"copy": lambda: ops.copy_(scratch, flat.data),
                "adamw_step": lambda: flat.adamw_step(LR, weight_decay=WD),
                "groups_1": grouped("groups_1", False), "groups_2": grouped("groups_2", False),
                "groups_lrd": grouped("groups_lrd", False), "groups_lrd_ema": grouped("groups_lrd", True),
                "ema_update": ema_alone, "lrd_plus_ema": lrd_plus_ema}
    if not a.skip_per_tensor:
        net2 = _vivit()
        opt = optim.AdamW(optim.param_groups(net2, LR, WD, layer_decay=LAYER_DECAY), lr=LR)
        for p in net2.parameters():
            p.grad = torch.randn(p.shape, generator=gen).cuda() * 0.02
        variants["per_tensor"] = opt.step
    times = _alternate(variants, a.rounds, a.window)
    n = flat.total
    res = {"elements": sum(p.numel() for p in flat.params), "flat_elements": n, "tensors": len(flat.params),
           "ngroups": {k: v[2] for k, v in tables.items()}}
    copy_rate = n * BYTES["copy"] / statistics.median(times["copy"])
    res["copy_rate_gbs"] = round(copy_rate / 1e9, 1)
    for k, ts in times.items():
        res[k] = _stats(ts)
        if k in BYTES:
            res[k]["bytes_per_element"] = BYTES[k]
            res[k]["floor_peak_us"] = round(n * BYTES[k] / (HBM_PEAK_GBS * 1e9) * 1e6, 2)
            res[k]["floor_copy_rate_us"] = round(n * BYTES[k] / copy_rate * 1e6, 2)
    med = {k: statistics.median(ts) for k, ts in times.items()}
    res["ratio_groups_lrd_to_adamw_step"] = round(med["groups_lrd"] / med["adamw_step"], 4)
    res["adamw_step_spread_us"] = round((max(times["adamw_step"]) - min(times["adamw_step"])) * 1e6, 2)
    res["fusion_saving_us"] = round((med["lrd_plus_ema"] - med["groups_lrd_ema"]) * 1e6, 2)
    return res


def bench_captured(a):
    from dvt_amd import optim
    from dvt_amd.dp import FlatParameters
    from dvt_amd.graph import capture_step
    g = torch.Generator().manual_seed(1130)
    x = torch.randn(8, 32, 3, 224, 224, generator=g).to(torch.bfloat16).cuda()
    y = (torch.rand(8, 19, generator=g) < 0.2).float().cuda()
    steps, held = {}, []
    for name in ("step_adamw", "step_groups_lrd", "step_groups_lrd_ema"):
        net = _vivit()
        flat = FlatParameters(net, compute_dtype=torch.bfloat16)
        flat.sync_compute_copy()
        seed = torch.full((), flat.loss_scale, device="cuda")
        lr_dev = torch.full((1,), LR, dtype=torch.float32, device="cuda")
        if name != "step_adamw":
            flat.set_param_groups(optim.param_groups(net, LR, WD, layer_decay=LAYER_DECAY))
        if name.endswith("_ema"):
            flat.enable_ema(0.9999)

        def step(net=net, flat=flat, seed=seed, lr_dev=lr_dev, uniform=(name == "step_adamw")):
            flat.zero_grad()
            loss, _ = net.loss(x, y)
            loss.backward(seed)
            flat.finish_backward()
            if uniform:
                flat.adamw_step(LR, weight_decay=WD)
            else:
                flat.adamw_groups_step(lr_dev)
            return loss
        steps[name] = step
        held.append((net, flat, seed, lr_dev))
    captured = {k: capture_step(fn, warmup=2) for k, fn in steps.items()}
    times = _alternate({k: replay for k, (replay, _) in captured.items()}, max(3, a.rounds // 2), a.window)
    torch.cuda.synchronize()
    res = {k: _stats(ts) for k, ts in times.items()}
    del captured, steps, held
    return res


def _kernel_label(name):
    """"adamw_groups_kernel<bf16, ema>" and the like from a kernel name of the trace, mangled or demangled; None for any
    other kernel"""
    base = next((k for k in KERNELS if k in name), None)
    if base is None:
        return None
    rest = name.split(base, 1)[1]
    mirror = ("bf16" if rest.startswith(("IDF16b", "<std::bfloat16_t", "<__bf16")) else
              "f16" if rest.startswith(("IDF16_", "<_Float16")) else "none" if rest.startswith(("If", "<float")) else None)
    if mirror is None:
        return base
    if base == "adamw_groups_kernel":
        return f"{base}<{mirror}, {'ema' if ('Lb1E' in rest[:12] or ', true>' in rest[:40]) else 'plain'}>"
    return f"{base}<{mirror}>"


def kernel_trace(directory):
    """Median / count of the durations (us) of the optimizer kernels in a rocprofv3 kernel-trace CSV under ``directory``,
    per kernel symbol (so per mirror type and kEma form)."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    dur = {}
    for f in files:
        for r in csv.DictReader(open(f)):
            short = _kernel_label(r["Kernel_Name"])
            if short is not None:
                dur.setdefault(short, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"median_us": round(statistics.median(v), 2), "p10_us": round(sorted(v)[len(v) // 10], 2),
                "p90_us": round(sorted(v)[(9 * len(v)) // 10], 2), "n": len(v)} for k, v in sorted(dur.items())}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.2)
    ap.add_argument("--skip-step", action="store_true")
    ap.add_argument("--skip-per-tensor", action="store_true")
    ap.add_argument("--kernel-trace", metavar="DIR", help="summarise a rocprofv3 kernel trace instead of timing")
    a = ap.parse_args()
    if a.kernel_trace:
        print(json.dumps({"kernel_trace": kernel_trace(a.kernel_trace)}))
        return 0
    if not torch.cuda.is_available():
        sys.exit("bench_optim_groups: needs the MI355X; there is nothing to measure on a CPU")
    import dvt_amd
    dvt_amd._lib.load()
    res = {"device": torch.cuda.get_device_name(0), "rounds": a.rounds, "window_s": a.window, "hbm_peak_gbs": HBM_PEAK_GBS,
           "lr": LR, "weight_decay": WD, "layer_decay": LAYER_DECAY}
    res["steps"] = bench_steps(a)
    if not a.skip_step:
        res["captured"] = bench_captured(a)
    print(json.dumps(res))
    return 0


if __name__ == "__main__":
    sys.exit(main())
