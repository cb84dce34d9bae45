#!/usr/bin/env python3
"""Measure stochastic depth on the MI355X: the sequence gather and scatter-add, the draws, and the training step.

    python tools/bench_drop_path.py [--out profiles/drop_path.md] [--rounds 7] [--window 0.5] [--rates 0.1 0.3] [--skip-step]

Timing as in tools/bench_patch_dropout.py: device events around windows of at least ``--window`` seconds of back-to-back
calls, after a warm-up of every variant; the variants alternate within one process, round by round, and a variant's figure
is the median over the rounds of its window means.

1. Kernels at the space stack of the metric shape, x [256, 197, 512] bf16 (51.6 MB): ``ops.seq_gather`` and
   ``ops.seq_scatter_add`` at k / S = 1.0, 0.9, 0.75 and 0.5 with the bytes each moves (the gather reads and writes k rows;
   the scatter-add reads S + k rows and writes S), against the device copy rate measured in the same run (``ops.copy_`` of
   the same tensor) and ``ops.add`` on the full tensor (what a residual add costs when it is not fused into a GEMM).
2. The draw launches: ``ops.drop_path_draw`` at S = 256 and ``ops.keep_draw(1, 256, k)``.
3. Step, ``ViViT.loss`` forward + backward at the metric shape (bf16): ``drop_path`` 0 and each rate of ``--rates`` in
   ``subset`` and in ``bernoulli`` mode, each replayed from a captured hipGraph (``F.next_step()`` inside: new subsets per
   replay): ms / step, the ratio to ``drop_path = 0``, peak allocated memory of an eager step.

Lifetimes: the generator is seeded once, before anything is built, and never again.  Every step closure (with its model,
``FlatParameters`` and seed tensor bound as defaults), the inputs and the graphs' outputs stay referenced until the last
replay has been followed by a ``torch.cuda.synchronize()``: a captured graph owns only what was allocated during capture.
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

FRACTIONS = (1.0, 0.9, 0.75, 0.5)


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
    torch.cuda.synchronize()
    return out


def bench_kernels(rounds, seconds):
    from dvt_amd import ops
    S, N, d = 256, 197, 512
    g = torch.Generator().manual_seed(1130)
    x = torch.randn(S, N, d, generator=g).to(torch.bfloat16).cuda()
    y_full = torch.randn(S, N, d, generator=g).to(torch.bfloat16).cuda()
    dst = torch.empty_like(x)
    row = N * d * x.element_size()
    state = torch.tensor([7, 0], dtype=torch.int64, device="cuda")
    variants = {"copy_ (device copy rate)": lambda: ops.copy_(dst, x), "add": lambda: ops.add(x, y_full)}
    nbytes = {"copy_ (device copy rate)": 2 * S * row, "add": 3 * S * row}
    held = []
    for frac in FRACTIONS:
        k = int(round(S * frac))
        keep, slot = ops.keep_draw(1, S, k, state, 0)
        keep, slot = keep.view(k), slot.view(S)
        y = y_full[:k].contiguous()
        # checked at the size that is timed: the gathered rows are the rows keep names; the scatter-add changes only those
        got = ops.seq_gather(x, keep, 1.0)
        assert torch.equal(got, x[keep.long()]), frac
        out = ops.seq_scatter_add(x, y, slot, 1.0)
        dropped = (slot < 0).nonzero().flatten()
        assert torch.equal(out[dropped], x[dropped]) and dropped.numel() == S - k
        held.append((keep, slot, y))
        variants[f"seq_gather k/S {frac}"] = lambda keep=keep: ops.seq_gather(x, keep, 1.0)
        variants[f"seq_scatter_add k/S {frac}"] = lambda y=y, slot=slot: ops.seq_scatter_add(x, y, slot, S / k)
        nbytes[f"seq_gather k/S {frac}"] = 2 * k * row
        nbytes[f"seq_scatter_add k/S {frac}"] = (2 * S + k) * row
        del got, out
    times = _alternate(variants, rounds, seconds)
    copy_rate = nbytes["copy_ (device copy rate)"] / statistics.median(times["copy_ (device copy rate)"])
    lines = [f"Device copy rate in this run (`ops.copy_`, {2 * S * row / 1e6:.1f} MB moved): {copy_rate / 1e12:.2f} TB/s.", "",
             "| variant | median us | min us | max us | bytes moved | TB/s | share of the copy rate |", "|---|---|---|---|---|---|---|"]
    for name, v in times.items():
        med = statistics.median(v)
        lines.append(f"| `{name}` | {med * 1e6:.2f} | {min(v) * 1e6:.2f} | {max(v) * 1e6:.2f} | {nbytes[name]} | "
                     f"{nbytes[name] / med / 1e12:.2f} | {nbytes[name] / med / copy_rate:.2f} |")
    small = {"drop_path_draw S 256 p 0.1": lambda: ops.drop_path_draw(S, 0.1, state, 0),
             "keep_draw(1, 256, 231)": lambda: ops.keep_draw(1, S, 231, state, 0),
             "keep_draw(1, 256, 128)": lambda: ops.keep_draw(1, S, 128, state, 0)}
    times = _alternate(small, max(3, rounds // 2), min(seconds, 0.2))
    lines += ["", "The draw launches (event-timed back to back: host-bound at this size, an upper bound of the launch):", "",
              "| launch | median us | min us | max us |", "|---|---|---|---|"]
    for name, v in times.items():
        lines.append(f"| `{name}` | {statistics.median(v) * 1e6:.2f} | {min(v) * 1e6:.2f} | {max(v) * 1e6:.2f} |")
    del variants, small, held
    return lines


def bench_step(rounds, seconds, rates):
    from dvt_amd import functional as F
    from dvt_amd import ops
    from dvt_amd.dp import FlatParameters
    from dvt_amd.graph import capture_step
    from dvt_amd.models.vit import ViViT
    cdt, image, T, depth = torch.bfloat16, 224, 32, 4
    g = torch.Generator().manual_seed(1130)
    x = torch.randn(8, T, 3, image, image, generator=g).to(cdt).cuda()
    y = (torch.rand(8, 19, generator=g) < 0.2).float().cuda()
    rng_state = F._rng.tensor(x.device)                   # the one state tensor every captured draw addresses
    cases = [(0.0, "subset")] + [(p, m) for p in rates for m in ("subset", "bernoulli")]
    steps, peak, kept, held = {}, {}, {}, []
    for case in cases:
        p, mode = case
        ops._ws.clear()                                   # grow-only scratch of whatever ran before
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        torch.manual_seed(1130)
        net = ViViT(image, 16, 19, T, dim=512, depth=depth, heads=8, dim_head=64, compute_dtype=cdt, drop_path=p,
                    drop_path_mode=mode).cuda().train()
        flat = FlatParameters(net, compute_dtype=cdt)
        flat.sync_compute_copy()
        seed = torch.full((), flat.loss_scale, device="cuda")

        def step(net=net, flat=flat, seed=seed, x=x, y=y):
            flat.zero_grad()
            loss, _ = net.loss(x, y)
            loss.backward(seed)
            flat.finish_backward()
            F.next_step()                                 # device-side: the replayed graph draws new subsets every step
            return loss

        steps[case] = step
        held.append((net, flat, seed))
        rs = net.space_transformer.drop_path_rates
        kept[case] = " ".join(str(ViViT.drop_path_kept(8 * T, r)) for r in rs) if mode == "subset" else "256 (all)"
        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        peak[case] = (torch.cuda.max_memory_allocated() - before) / 2 ** 30
    # one captured hipGraph per variant; the closures, the models behind them and the graphs' outputs are held in `steps`,
    # `held` and `captured` until every replay has finished
    captured = {c: capture_step(fn, warmup=1) for c, fn in steps.items()}
    times = _alternate({c: replay for c, (replay, _) in captured.items()}, rounds, seconds)
    torch.cuda.synchronize()
    assert F._rng.state is rng_state                      # nobody re-seeded between capture and the last replay
    base = statistics.median(times[cases[0]])
    lines = ["Launch form: hipGraph replay of zero_grad + forward + loss + backward + next_step (no optimizer step), metric shape "
             "b 8, T 32, 224^2, depth 4, bf16.  `drop_path` is the rate of the last of the 8 layers; the space stack's four "
             "layers run at 0, 1/7, 2/7, 3/7 of it.", "",
             "| drop_path | mode | ms / step | min | max | ratio to drop_path = 0 | sequences a space layer's branches run on (of 256) "
             "| peak allocated GiB (model + step) |", "|---|---|---|---|---|---|---|---|"]
    for c in cases:
        med = statistics.median(times[c])
        lines.append(f"| {c[0]} | {c[1] if c[0] else '-'} | {med * 1e3:.3f} | {min(times[c]) * 1e3:.3f} | {max(times[c]) * 1e3:.3f} | "
                     f"{med / base:.3f} | {kept[c]} | {peak[c]:.2f} |")
    del times, captured                                   # the graphs first, after the synchronize above ...
    del steps, held, x, y, rng_state                      # ... then what they addressed
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None, help="write the report here as well (markdown)")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--window", type=float, default=0.5)
    ap.add_argument("--rates", type=float, nargs="+", default=[0.1, 0.3])
    ap.add_argument("--skip-step", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_drop_path: needs the MI355X; there is nothing to measure on a CPU")
    import dvt_amd
    dvt_amd._lib.load()
    dvt_amd.functional.manual_seed(1130)                  # once, before anything is built
    report = ["# Stochastic depth: measurements", "", f"Device: {torch.cuda.get_device_name(0)}; windows of >= {args.window} s, "
              f"{args.rounds} alternating rounds, device events (`python tools/bench_drop_path.py --rounds {args.rounds} "
              f"--window {args.window} --rates {' '.join(map(str, args.rates))}`).", "",
              "## Sequence gather and scatter-add: x [256, 197, 512] bf16", ""]
    report += bench_kernels(args.rounds, args.window)
    if not args.skip_step:
        report += ["", "## Step: ViViT.loss forward + backward", ""]
        report += bench_step(max(3, args.rounds // 2), args.window, args.rates)
    text = "\n".join(report) + "\n"
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)
    return 0


if __name__ == "__main__":
    sys.exit(main())
