#!/usr/bin/env python3
"""Measure the tubelet embedding on the MI355X: the gather against the per-frame gather, and the training step at
tubelet_size 1 and 2.

    python tools/bench_tubelet.py [--out profiles/tubelet_embed.md] [--rounds 7] [--window 0.5] [--skip-step]

Timing: device events around windows of at least ``--window`` seconds of back-to-back calls, after a warm-up of every
variant; the variants alternate within one process, round by round, and a variant's figure is the median over the rounds
of its window means.  The spread is what repeated timings of the SAME code show in this run: max - min of the per-frame
gather's window means.

1. Gather, metric clip [8, 32, 3, 224, 224], bf16 -> bf16: ``ops.patchify`` and ``ops.tubelet_patchify`` at pt 1, 2 and
   4 (pt = 1 is the per-frame launch under its other name).  The same bytes move along the same image rows, so the
   tubelet gather is held to the per-frame one: its median may exceed patchify's by no more than that spread (reported
   as held / missed; exit status 1 when missed).  The vector form (f32 -> f32) is timed after it and reported only.
2. Step, ``ViViT.loss`` forward + backward at the metric shape (bf16) and at BASELINE configs[4] (T = 64, 288^2, fp16,
   activation checkpointing), tubelet_size 1 and 2, each replayed from a captured hipGraph: ms / step, space-stack rows,
   peak allocated memory of an eager step above what was allocated before the model was built.  Reported only.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s


def _window(fn, seconds, calls_hint):
    """Mean device time of one call of fn over a window of >= seconds -> (seconds per call, calls)."""
    calls = max(1, calls_hint)
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
        _, hint[name] = _window(fn, min(seconds, 0.1), 1)
    out = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            t, hint[name] = _window(fn, seconds, hint[name])
            out[name].append(t)
    return out


def bench_gather(rounds, seconds):
    from dvt_amd import ops
    g = torch.Generator().manual_seed(1130)
    x = torch.randn(8, 32, 3, 224, 224, generator=g).to(torch.bfloat16).cuda()
    nbytes = 2 * x.numel() * x.element_size()
    ref = ops.patchify(x, 16, torch.bfloat16).view(8, 32, 196, 768)
    for pt in (1, 2, 4):   # the outputs are the per-frame vectors regrouped: checked at the size that is timed
        got = ops.tubelet_patchify(x, 16, pt, torch.bfloat16).view(8, 32 // pt, 196, pt, 768)
        assert torch.equal(got, ref.view(8, 32 // pt, pt, 196, 768).transpose(2, 3)), pt
    variants = {"patchify": lambda: ops.patchify(x, 16, torch.bfloat16),
                "tubelet pt=1": lambda: ops.tubelet_patchify(x, 16, 1, torch.bfloat16),
                "tubelet pt=2": lambda: ops.tubelet_patchify(x, 16, 2, torch.bfloat16),
                "tubelet pt=4": lambda: ops.tubelet_patchify(x, 16, 4, torch.bfloat16)}
    times = _alternate(variants, rounds, seconds)
    base = times["patchify"]
    spread = max(base) - min(base)
    med = {k: statistics.median(v) for k, v in times.items()}
    lines = ["| variant | median us | min us | max us | bytes (in + out) | share of the 8 TB/s HBM peak | within the spread |",
             "|---|---|---|---|---|---|---|"]
    held = True
    for k, v in times.items():
        ok = med[k] - med["patchify"] <= spread
        held &= ok
        lines.append(f"| `{k}` | {med[k] * 1e6:.3f} | {min(v) * 1e6:.3f} | {max(v) * 1e6:.3f} | {nbytes} | "
                     f"{nbytes / med[k] / HBM_PEAK:.3f} | {'-' if k == 'patchify' else 'held' if ok else 'MISSED'} |")
    lines.append("")
    lines.append(f"Spread of the repeated `patchify` windows in this run (max - min over {rounds} rounds): "
                 f"{spread * 1e6:.3f} us.  Condition (tubelet median - patchify median <= spread): "
                 f"{'held' if held else 'MISSED'}.")
    # the vector form (what an fp32 destination takes): reported, not gated -- it is on no measured path
    xf = torch.randn(8, 32, 3, 224, 224, generator=g).cuda()
    vt = _alternate({"v": lambda: ops.patchify(xf, 16, torch.float32)}, max(3, rounds // 2), seconds)["v"]
    lines.append(f"Vector form, `patchify` f32 -> f32 on the same shape ({4 * xf.numel() * 2} bytes): median "
                 f"{statistics.median(vt) * 1e6:.3f} us (min {min(vt) * 1e6:.3f}, max {max(vt) * 1e6:.3f}); reported only.")
    return lines, held


def bench_step(rounds, seconds):
    from dvt_amd import ops
    from dvt_amd.dp import FlatParameters
    from dvt_amd.graph import capture_step
    from dvt_amd.models.vit import ViViT
    lines = ["Launch form: hipGraph replay of forward + loss + backward (no optimizer step).", "",
             "| shape | tubelet_size | ms / step | space-stack rows | peak allocated GiB (model + step) |", "|---|---|---|---|---|"]
    shapes = [("metric: b 8, T 32, 224^2, bf16", dict(image=224, T=32), torch.bfloat16, False),
              ("configs[4]: b 8, T 64, 288^2, fp16, checkpointing", dict(image=288, T=64), torch.float16, True)]
    for label, cfg, cdt, ckpt in shapes:
        g = torch.Generator().manual_seed(1130)
        x = torch.randn(8, cfg["T"], 3, cfg["image"], cfg["image"], generator=g).to(cdt).cuda()
        y = (torch.rand(8, 19, generator=g) < 0.2).float().cuda()
        steps, rows, peak = {}, {}, {}
        for pt in (1, 2):
            # a variant's own footprint: what its step allocates above what was there before the model was built
            # (parameters, gradients, activations, workspaces; the input clip is not in the figure)
            ops._ws.clear()                   # grow-only scratch of whatever ran before: it would count for this variant
            torch.cuda.empty_cache()
            before = torch.cuda.memory_allocated()
            torch.manual_seed(1130)
            net = ViViT(cfg["image"], 16, 19, cfg["T"], dim=512, depth=4, heads=8, dim_head=64, compute_dtype=cdt,
                        activation_checkpointing=ckpt, tubelet_size=pt).cuda().train()
            flat = FlatParameters(net, compute_dtype=cdt)
            flat.sync_compute_copy()
            seed = flat.enable_loss_scaling(init_scale=4096.0, growth_interval=1000) if cdt == torch.float16 else \
                torch.full((), flat.loss_scale, device="cuda")

            def step(net=net, flat=flat, seed=seed):
                flat.zero_grad()
                loss, _ = net.loss(x, y)
                loss.backward(seed)
                flat.finish_backward()
                return loss

            steps[pt] = step
            rows[pt] = 8 * (cfg["T"] // pt) * ((cfg["image"] // 16) ** 2 + 1)
            step()
            torch.cuda.synchronize()
            torch.cuda.reset_peak_memory_stats()
            step()
            torch.cuda.synchronize()
            peak[pt] = (torch.cuda.max_memory_allocated() - before) / 2 ** 30
        # timed as the product runs a step: one captured hipGraph per variant, replayed (launched one by one from Python
        # the host cannot keep the device fed at the metric shape)
        times = _alternate({pt: capture_step(fn, warmup=1)[0] for pt, fn in steps.items()}, rounds, seconds)
        for pt in (1, 2):
            lines.append(f"| {label} | {pt} | {statistics.median(times[pt]) * 1e3:.2f} | {rows[pt]} | {peak[pt]:.2f} |")
        del steps, times, x               # the graphs' pools go with them
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the report here as well (markdown)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_tubelet: needs the MI355X; there is nothing to measure on a CPU")
    import dvt_amd
    dvt_amd._lib.load()
    report = ["# Tubelet embedding: measurements", "", f"Device: {torch.cuda.get_device_name(0)}; windows of >= {args.window} s, "
              f"{args.rounds} alternating rounds, device events (tools/bench_tubelet.py).", "",
              "## Gather: metric clip [8, 32, 3, 224, 224], bf16 -> bf16", ""]
    lines, held = bench_gather(args.rounds, args.window)
    report += lines
    if not args.skip_step:
        report += ["", "## Step: ViViT.loss forward + backward (reported, not gated)", ""]
        report += bench_step(max(3, args.rounds // 2), args.window)
    text = "\n".join(report) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0 if held else 1


if __name__ == "__main__":
    sys.exit(main())
