"""Mixup / CutMix of a clip batch, the mixed targets and the soft-target cross-entropy on the MI355X, timed with hipEvents:
eager launches only (no graph is captured), the forms of one group taken in turn within every repeat, the median and the
range of the repeats reported.  Every tensor a timed call reads, writes or returns -- the results the forms allocate and the
``x.flip(0)`` of the torch forms included -- is appended to ``KEEP`` and lives until the process ends.  So that holding
them does not put a device allocation inside every timed call, the caching allocator is filled beforehand with as many
blocks of each size as the run will ask for (``_reserve``).  One JSON line.

    python tools/bench_mix.py [--warmup 5] [--steps 10] [--repeats 5]        # holds about 22 GB at these counts
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_mix.py --steps 5 --repeats 1
    python tools/bench_mix.py --kernel-trace DIR        # per-kernel, per-grid medians of that trace, no GPU work

The event-timed figures include the host's time to issue a call wherever that exceeds the kernel's (the small shapes); the
kernel trace gives the kernels' own durations.

Per clip shape ([8, 32, 3, 224, 224], the metric clip, and FrameTransformer's [2, 156, 3, 112, 112]; bf16):
  mixup_in_place / mixup_out_of_place / cutmix_in_place (lam = 0.5: a tube box of half the frame)    ops.clips_mix
  patchify          ops.patchify on the same clip: the in-tree streaming kernel that moves the same bytes once each way
  torch_mixup       x.mul(lam).add_(x.flip(0), alpha=1 - lam): three eager launches, >= 2.5 x the bytes
  torch_cutmix      x[..., y0:y1, x0:x1] = x.flip(0)[..., y0:y1, x0:x1]
  floor_*           the bytes the form must move at 8 TB/s (HBM peak) and at 6.29 TB/s (the measured float4 copy rate)
and at [256, 305]: ops.targets_mix, ops.ce_soft_fwd + ce_soft_bwd against their torch-eager forms.
"""
from __future__ import annotations

import argparse
import csv
import glob
import json
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK_GBS, HBM_COPY_GBS = 8000.0, 6290.0
SHAPES = {"metric_clip": (8, 32, 3, 224, 224), "frame_transformer": (2, 156, 3, 112, 112)}
KEEP = []                                   # every tensor a timed call reads or writes lives as long as the process


def _keep(t):
    KEEP.append(t)
    return t


def _reserve(nbytes, count):
    """``count`` blocks of ``nbytes`` allocated and released into the caching allocator's pool: later requests of that size
    are served from it, however many of their results are held"""
    blocks = [torch.empty(nbytes, dtype=torch.uint8, device="cuda") for _ in range(count)]
    del blocks


def _time_group(forms, warmup, steps, repeats):
    """forms: {name: fn}.  Each repeat times every form in turn (``steps`` event-timed calls each) -> {name: stats}."""
    for fn in forms.values():
        for _ in range(warmup):
            fn()
    torch.cuda.synchronize()
    med = {k: [] for k in forms}
    for _ in range(repeats):
        for name, fn in forms.items():
            ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(steps)]
            for a, b in ev:
                a.record()
                fn()
                b.record()
            torch.cuda.synchronize()
            ms = sorted(a.elapsed_time(b) for a, b in ev)
            med[name].append(ms[len(ms) // 2] * 1e3)
    out = {}
    for name, v in med.items():
        s = sorted(v)
        out[name] = {"median_us": round(s[len(s) // 2], 2), "min_us": round(s[0], 2), "max_us": round(s[-1], 2), "repeats": len(s)}
    return out


KERNELS = ("clips_mix_kernel", "patchify_p16_fwd_kernel", "targets_mix_kernel", "ce_soft_fwd_kernel", "ce_soft_bwd_kernel")


def kernel_trace(directory):
    """Median / count of the durations (us) of this tool's HIP kernels in a rocprofv3 kernel-trace CSV under ``directory``,
    one entry per (kernel, grid size): the forms of ops.clips_mix differ in their grids."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    dur = {}
    for r in csv.DictReader(open(files[0])):
        for k in KERNELS:
            if k in r["Kernel_Name"]:
                grid = "x".join(str(r.get(f"Grid_Size_{a}", r.get(f"Grid_Size{a}", "?"))) for a in ("X", "Y"))
                dur.setdefault(f"{k} grid {grid}", []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"median_us": round(sorted(v)[len(v) // 2], 2), "min_us": round(min(v), 2), "n": len(v)} for k, v in dur.items()}


def _floor(nbytes):
    return {"bytes": int(nbytes), "us_at_8TBs": round(nbytes / (HBM_PEAK_GBS * 1e9) * 1e6, 2),
            "us_at_6.29TBs": round(nbytes / (HBM_COPY_GBS * 1e9) * 1e6, 2)}


def bench_clip(ops, shape, a):
    B, T, C, H, W = shape
    x = _keep(torch.randn(shape, device="cuda").to(torch.bfloat16))
    out = _keep(torch.empty_like(x))
    flip = list(range(B - 1, -1, -1))
    side = int(H * math.sqrt(0.5))
    y0, x0 = (H - side) // 2, (W - side) // 2
    mix_tab = torch.tensor([[p, 1, 0, T, 0, H, 0, W] for p in flip], dtype=torch.int32)
    cut_tab = torch.tensor([[p, 2, 0, T, y0, y0 + side, x0, x0 + side] for p in flip], dtype=torch.int32)
    lam = torch.full((B,), 0.5)
    patch = 16
    forms = {
        "mixup_in_place": lambda: ops.clips_mix(x, mix_tab, lam),
        "mixup_out_of_place": lambda: ops.clips_mix(x, mix_tab, lam, out=out),
        "cutmix_in_place": lambda: ops.clips_mix(x, cut_tab, lam),
        "patchify": lambda: _keep(ops.patchify(x, patch, torch.bfloat16)),
        "torch_mixup": lambda: _keep(x.mul(0.5)).add_(_keep(x.flip(0)), alpha=0.5),
        "torch_cutmix": lambda: x[:, :, :, y0:y0 + side, x0:x0 + side].copy_(_keep(x.flip(0))[:, :, :, y0:y0 + side, x0:x0 + side]),
    }
    _reserve(x.numel() * 2, 4 * (a.warmup + a.steps * a.repeats))       # patchify's rows, the product, two flips: per round
    res = _time_group(forms, a.warmup, a.steps, a.repeats)
    nbytes = x.numel() * 2
    box = B * T * C * side * side * 2
    res["floor_mixup"] = _floor(2 * nbytes)                      # every byte read once and written once, either way
    res["floor_cutmix"] = _floor(2 * box)
    res["floor_patchify"] = _floor(2 * nbytes)
    res["box"] = [y0, y0 + side, x0, x0 + side]
    for k, ref in (("mixup_in_place", "torch_mixup"), ("mixup_out_of_place", "torch_mixup"), ("cutmix_in_place", "torch_cutmix")):
        res[k]["speedup_over_torch"] = round(res[ref]["median_us"] / res[k]["median_us"], 2)
        res[k]["faster_than_torch"] = res[k]["median_us"] < res[ref]["median_us"]
    for k in ("mixup_in_place", "mixup_out_of_place"):
        res[k]["ratio_to_patchify"] = round(res[k]["median_us"] / res["patchify"]["median_us"], 2)
    return res


def bench_targets(ops, a):
    M, Ccls = 256, 305
    g = torch.Generator().manual_seed(0)
    labels = _keep(torch.randint(0, Ccls, (M,), generator=g).cuda())
    logits = _keep(torch.randn(M, Ccls, generator=g).cuda())
    flip = list(range(M - 1, -1, -1))
    table = torch.tensor([[p, 1, 0, 0, 0, 0, 0, 0] for p in flip], dtype=torch.int32)
    lam = torch.rand(M, generator=g)
    lam_dev = _keep(lam.cuda().unsqueeze(1))
    targets = _keep(ops.targets_mix(table, lam, labels=labels, num_classes=Ccls, smoothing=0.1))
    gloss = _keep(torch.ones(1, device="cuda"))
    leaf = _keep(logits.clone().requires_grad_(True))

    def torch_targets():
        y = torch.nn.functional.one_hot(labels, Ccls).float() * 0.9 + 0.1 / Ccls
        return _keep(y * lam_dev + y.flip(0) * (1 - lam_dev))

    def hip_ce():
        loss, lse = ops.ce_soft_fwd(logits, targets)
        return _keep((loss, lse, ops.ce_soft_bwd(logits, targets, lse, gloss)))

    def torch_ce():
        leaf.grad = None
        loss = torch.sum(-targets * torch.log_softmax(leaf, -1), -1).mean()
        loss.backward()
        return _keep(loss)

    _reserve(M * Ccls * 4, 4 * (a.warmup + a.steps * a.repeats))        # the mixed rows (twice), dlogits; one spare
    forms = {"targets_mix": lambda: _keep(ops.targets_mix(table, lam, labels=labels, num_classes=Ccls,
                                                                               smoothing=0.1)),
             "torch_targets": torch_targets, "ce_soft_fwd_bwd": hip_ce, "torch_soft_ce_fwd_bwd": torch_ce}
    return _time_group(forms, a.warmup, a.steps, a.repeats)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--kernel-trace", metavar="DIR", help="summarise a rocprofv3 kernel trace instead of timing")
    a = ap.parse_args()
    if a.kernel_trace:
        print(json.dumps({"kernel_trace": kernel_trace(a.kernel_trace)}))
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_mix.py times the MI355X: no GPU visible, nothing measured")
    from dvt_amd import ops
    res = {"warmup": a.warmup, "steps": a.steps, "repeats": a.repeats, "dtype": "bf16"}
    for name, shape in SHAPES.items():
        res[name] = {"shape": list(shape), **bench_clip(ops, shape, a)}
    res["targets_256x305"] = bench_targets(ops, a)
    res["clips_mix_faster_than_torch"] = all(res[n][k]["faster_than_torch"] for n in SHAPES
                                             for k in ("mixup_in_place", "mixup_out_of_place", "cutmix_in_place"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
