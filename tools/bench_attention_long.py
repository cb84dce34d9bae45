#!/usr/bin/env python3
"""Measure the streamed attention kernels (attn_long_* of csrc/attention.hip) on the MI355X.

    python tools/bench_attention_long.py [--out profiles/attention_long.md] [--rounds 5] [--window 0.3] [--skip-step]

Timing as in tools/bench_mae.py: device events around windows of at least ``--window`` seconds of back-to-back calls, after
a warm-up of every variant; the variants alternate within one process, round by round; a variant's figure is the median
over the rounds of its window means and its spread the min and max of them.

1. Kernels: bf16, [8, 8, L, 64] on the packed [B, L, 3, H, dh] layout at L = 785, 1569, 3137, forward and backward, through
   ``ops.attention_long_fwd`` / ``_bwd`` and, in the same run, through ``ops.attention_fwd`` / ``_bwd`` (the generic kernels:
   what these shapes launched before); and the resident kernels as the FLOP-rate yardstick: ``attention_fwd`` at
   L = 640 (the online family) and ``attention_bwd`` at L = 608 (the kernel pair: its Q / dO images with their statistics
   take 264 B per query row of the 160 KiB, so 608 is the longest padded length it reaches; 640 is already generic).
   FLOPs counted as the algorithm's: 4 L^2 dh per (b, h) forward, 10 L^2 dh backward (5 products; the pair and the
   streamed backward issue 7).
2. Step: ``JointViViT.loss`` forward + backward at the metric clip [8, 32, 3, 224, 224] with ``tubelet_size=2`` (3137 tokens
   per clip; dim 512, depth 4, 8 heads), replayed from a captured hipGraph, beside ``ViViT.loss`` of the same geometry in
   the same run, and the same JointViViT step with ``functional.ATTN_LONG = False`` (eager, one window: the generic route).
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

B, H, DH = 8, 8, 64
LENGTHS = (785, 1569, 3137)
YARD = {"forward": 640, "backward": 608}          # the longest lengths of the online forward and of the kernel pair


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
        for _ in range(2):
            fn()
        torch.cuda.synchronize()
        _, hint[name] = _window(fn, min(seconds, 0.1), 1)
    out = {name: [] for name in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            t, hint[name] = _window(fn, seconds, hint[name])
            out[name].append(t)
    torch.cuda.synchronize()
    return out


def bench_kernels(rounds, seconds):
    from dvt_amd import ops
    g = torch.Generator().manual_seed(1130)
    scale = DH ** -0.5
    variants, flops, held = {}, {}, []
    for L in tuple(sorted(set(YARD.values()))) + LENGTHS:
        qkv = (torch.randn(B, L, 3, H, DH, generator=g) * 0.7).to(torch.bfloat16).cuda()
        q, k, v = (qkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        o = torch.empty(B, L, H, DH, dtype=torch.bfloat16, device="cuda").permute(0, 2, 1, 3)
        do = torch.randn(B, L, H, DH, generator=g).to(torch.bfloat16).cuda().permute(0, 2, 1, 3)
        dqkv = torch.empty_like(qkv)
        dq, dk, dv = (dqkv[:, :, i].permute(0, 2, 1, 3) for i in range(3))
        lse = torch.empty(B, H, L, dtype=torch.float32, device="cuda")
        held.append((qkv, o, do, dqkv, lse))
        routes = [("resident", ops.attention_fwd, ops.attention_bwd)] if L in YARD.values() else \
            [("streamed", ops.attention_long_fwd, ops.attention_long_bwd), ("generic", ops.attention_fwd, ops.attention_bwd)]
        for route, fwd, bwd in routes:
            fwd(q, k, v, o, scale, lse=lse)               # lse and o of this route before its backward is timed
            passes = ("forward", "backward")
            if route == "resident":
                passes = tuple(pas for pas in passes if YARD[pas] == L)
                pf, pb = ops.attention_plan(q, k, v, o), ops.attention_plan(q, k, v, o, bwd=True, do=do)
                assert pf.family == "online" and (pb.family == "pair" or "backward" not in passes), (pf, pb)
            elif route == "generic":
                assert ops.attention_plan(q, k, v, o).family == "generic"
            if "forward" in passes:
                variants[f"{route} forward L {L}"] = lambda fwd=fwd, q=q, k=k, v=v, o=o, lse=lse: fwd(q, k, v, o, scale, lse=lse)
                flops[f"{route} forward L {L}"] = 4.0 * B * H * L * L * DH
            if "backward" in passes:
                variants[f"{route} backward L {L}"] = lambda bwd=bwd, q=q, k=k, v=v, o=o, lse=lse, do=do, dq=dq, dk=dk, dv=dv: bwd(
                    q, k, v, o, lse, do, dq, dk, dv, scale)
                flops[f"{route} backward L {L}"] = 10.0 * B * H * L * L * DH
    times = _alternate(variants, rounds, seconds)
    med = {n: statistics.median(v) for n, v in times.items()}
    rate = {n: flops[n] / med[n] / 1e12 for n in times}
    lines = ["| launch | median ms | min ms | max ms | GFLOP | TFLOP/s |", "|---|---|---|---|---|---|"]
    for n, v in times.items():
        lines.append(f"| {n} | {med[n] * 1e3:.3f} | {min(v) * 1e3:.3f} | {max(v) * 1e3:.3f} | {flops[n] / 1e9:.1f} | {rate[n]:.1f} |")
    lines += ["", "(a) against the generic route, and (b) the FLOP rate against the resident kernels (forward at L = 640, "
              "backward at L = 608) less the spread of the streamed launch's own repeats:", "",
              "| pass | L | streamed ms | generic ms | speed-up | streamed TFLOP/s | its spread | resident TFLOP/s | (a) | (b) |",
              "|---|---|---|---|---|---|---|---|---|---|"]
    for pas in ("forward", "backward"):
        yard = rate[f"resident {pas} L {YARD[pas]}"]
        for L in LENGTHS:
            s, gname = f"streamed {pas} L {L}", f"generic {pas} L {L}"
            lo, hi = flops[s] / max(times[s]) / 1e12, flops[s] / min(times[s]) / 1e12
            a = "met" if max(times[s]) < min(times[gname]) else "**missed**"
            b = "met" if rate[s] >= yard - (hi - lo) else "**missed**"
            lines.append(f"| {pas} | {L} | {med[s] * 1e3:.3f} | {med[gname] * 1e3:.3f} | {med[gname] / med[s]:.1f}x | {rate[s]:.1f} | "
                         f"{lo:.1f} .. {hi:.1f} | {yard:.1f} | {a} | {b} |")
    del variants, held
    return lines


def bench_step(rounds, seconds):
    from dvt_amd import functional as F
    from dvt_amd import ops
    from dvt_amd.dp import FlatParameters
    from dvt_amd.graph import capture_step
    from dvt_amd.models import JointViViT, ViViT
    cdt = torch.bfloat16
    Bc, T, IMAGE, P = 8, 32, 224, 16
    g = torch.Generator().manual_seed(1130)
    x = torch.randn(Bc, T, 3, IMAGE, IMAGE, generator=g).to(cdt).cuda()
    y = (torch.rand(Bc, 19, generator=g) < 0.2).float().cuda()
    steps, held, peak = {}, [], {}
    for name, cls in (("ViViT.loss tubelet_size 2 (factorised: 16 x 197 + 17 tokens)", ViViT),
                      ("JointViViT.loss tubelet_size 2 (3137 tokens)", JointViViT)):
        ops._ws.clear()
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        torch.manual_seed(1130)
        net = cls(IMAGE, P, 19, T, dim=512, depth=4, heads=8, dim_head=64, compute_dtype=cdt, tubelet_size=2).cuda().train()
        flat = FlatParameters(net, compute_dtype=cdt)
        flat.sync_compute_copy()
        seed = torch.full((), flat.loss_scale, device="cuda")

        def step(net=net, flat=flat, seed=seed):
            flat.zero_grad()
            loss = net.loss(x, y)[0]
            loss.backward(seed)
            flat.finish_backward()
            return loss

        steps[name] = step
        held.append((net, flat, seed))
        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        peak[name] = (torch.cuda.max_memory_allocated() - before) / 2 ** 30
    joint = steps["JointViViT.loss tubelet_size 2 (3137 tokens)"]
    F.ATTN_LONG = False                                   # the generic route, eager: one window is enough to see the cliff
    try:
        joint()
        torch.cuda.synchronize()
        generic, _ = _window(joint, min(seconds, 0.2), 1)
    finally:
        F.ATTN_LONG = True
    eager, _ = _window(joint, seconds, 2)
    captured = {name: capture_step(fn, warmup=1) for name, fn in steps.items()}
    times = _alternate({name: replay for name, (replay, _) in captured.items()}, rounds, seconds)
    torch.cuda.synchronize()
    lines = ["Launch form: hipGraph replay of zero_grad + forward + loss + backward (no optimizer step); b 8, T 32, 224^2, P 16, "
             "bf16, dim 512, depth 4, 8 heads.", "",
             "| step | ms / step | min | max | peak allocated GiB (model + step) |", "|---|---|---|---|---|"]
    for name in steps:
        v = times[name]
        lines.append(f"| {name} | {statistics.median(v) * 1e3:.3f} | {min(v) * 1e3:.3f} | {max(v) * 1e3:.3f} | {peak[name]:.2f} |")
    lines += ["", f"The JointViViT step eager: {eager * 1e3:.2f} ms with the streamed kernels, {generic * 1e3:.2f} ms with "
              f"`functional.ATTN_LONG = False` (the generic kernels in the three dense layers)."]
    del times, captured
    del steps, held, x, y
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the report here as well (markdown)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_attention_long: needs the MI355X; there is nothing to measure on a CPU")
    import dvt_amd
    from dvt_amd import ops
    dvt_amd._lib.load()
    dvt_amd.functional.manual_seed(1130)
    z = torch.zeros(1, 3137, 3, 1, DH, dtype=torch.bfloat16)
    plan = ops.attention_long_plan(*(z[:, :, i].permute(0, 2, 1, 3) for i in range(3)), z[:, :, 0].permute(0, 2, 1, 3), bwd=True)
    report = ["# Streamed attention (attn_long_*): measurements", "",
              f"Device: {torch.cuda.get_device_name(0)}; windows of >= {args.window} s, {args.rounds} alternating rounds, device "
              f"events (`python tools/bench_attention_long.py --rounds {args.rounds} --window {args.window}`).", "",
              f"Plan: {plan.q_block} query rows per workgroup and {plan.k_chunk} keys per chunk (forward, dq), {plan.k_block} key "
              f"rows and {plan.q_chunk} queries per chunk (dk/dv); {plan.waves} waves, {plan.ring} chunk buffers, "
              f"{plan.lds} / {plan.lds2} B of LDS.", "",
              f"## Kernels: bf16, [{B}, {H}, L, {DH}], packed layout", ""]
    report += bench_kernels(args.rounds, args.window)
    if not args.skip_step:
        report += ["", "## Step: forward + backward at the metric clip", ""]
        report += bench_step(max(3, args.rounds // 2), args.window)
    text = "\n".join(report) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
