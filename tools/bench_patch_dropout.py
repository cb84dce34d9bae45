#!/usr/bin/env python3
"""Measure patch dropout on the MI355X: the kept gather and its adjoint, the small launches, and the training step.

    python tools/bench_patch_dropout.py [--out profiles/patch_dropout.md] [--rounds 7] [--window 0.5] [--skip-step]

Timing as in tools/bench_tubelet.py: device events around windows of at least ``--window`` seconds of back-to-back calls,
after a warm-up of every variant; the variants alternate within one process, round by round, and a variant's figure is the
median over the rounds of its window means.

1. Gather, metric clip [8, 32, 3, 224, 224], bf16 -> bf16: ``ops.patchify_keep`` and ``ops.patchify_keep_bwd`` at keep
   fractions 1.0, 0.5 and 0.25 (tube rows) against ``ops.patchify`` / ``ops.patchify_bwd`` on the same clip, with the bytes
   each actually moves (the forward reads and writes the kept patches; the adjoint reads them and writes the whole clip)
   and the share of the 6.29 TB/s float4 copy rate profiles/mixup.md measured on this part.
2. The four small launches at the metric shape: ``keep_select``, ``keep_draw`` (tube), ``tokens_assemble_keep_fwd`` and
   ``tokens_assemble_keep_bwd`` at keep fraction 0.5.
3. Step, ``ViViT.loss`` forward + backward at the metric shape (bf16) for ``patch_dropout`` 0, 0.5 and 0.75 in tube mode,
   each replayed from a captured hipGraph (``F.next_step()`` inside: a new subset per replay): ms / step, space-stack rows,
   the ratio to ``patch_dropout = 0``, peak allocated memory of an eager step.

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

COPY_RATE = 6.29e12    # bytes / s: the measured float4 copy rate of this part (profiles/mixup.md)
FRACTIONS = (1.0, 0.5, 0.25)


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


def _row(name, times, nbytes):
    med = statistics.median(times)
    return (f"| `{name}` | {med * 1e6:.2f} | {min(times) * 1e6:.2f} | {max(times) * 1e6:.2f} | {nbytes} | "
            f"{nbytes / med / 1e12:.2f} | {nbytes / med / COPY_RATE:.2f} |")


def _tube_keep(b, t, n, k, seed):
    """keep / slot [b t, k] / [b t, n] of a tube draw at a fixed counter (its own state tensor: the model's is not touched)."""
    from dvt_amd import ops
    state = torch.tensor([seed, 0], dtype=torch.int64, device="cuda")
    return ops.keep_draw(b, n, k, state, 0, rows_per=t)


def bench_gather(rounds, seconds):
    from dvt_amd import ops
    b, t, n, P = 8, 32, 196, 16
    g = torch.Generator().manual_seed(1130)
    x = torch.randn(b, t, 3, 224, 224, generator=g).to(torch.bfloat16).cuda()
    full = ops.patchify(x, P, torch.bfloat16)
    dfull = torch.randn(full.shape, generator=g).to(torch.bfloat16).cuda()
    clip_bytes = x.numel() * x.element_size()
    fwd = {"patchify": lambda: ops.patchify(x, P, torch.bfloat16)}
    bwd = {"patchify_bwd": lambda: ops.patchify_bwd(dfull, x.shape, P, torch.bfloat16)}
    fwd_bytes, bwd_bytes = {"patchify": 2 * clip_bytes}, {"patchify_bwd": 2 * clip_bytes}
    held = []                                           # every tensor a timed closure reads, until the timing is over
    for frac in FRACTIONS:
        k = int(n * frac)
        keep, slot = _tube_keep(b, t, n, k, 7)
        rows = ops.patchify_keep(x, P, 1, keep, torch.bfloat16)
        # checked at the size that is timed: the rows keep names of the full gather, and the adjoint's zeros
        want = full.view(b * t, n, -1).gather(1, keep.long()[:, :, None].expand(b * t, k, full.shape[1])).reshape(b * t * k, -1)
        assert torch.equal(rows, want), frac
        dout = dfull[:rows.shape[0]].contiguous()
        dx = ops.patchify_keep_bwd(dout, x.shape, P, 1, slot, torch.bfloat16)
        back = ops.patchify(dx, P, torch.bfloat16).view(b * t, n, -1)
        assert torch.equal(back.gather(1, keep.long()[:, :, None].expand(b * t, k, full.shape[1])).reshape(b * t * k, -1), dout)
        assert int((back != 0).any(-1).sum()) <= b * t * k
        kept_bytes = rows.numel() * rows.element_size()
        held.append((keep, slot, dout))
        fwd[f"patchify_keep {frac}"] = lambda keep=keep: ops.patchify_keep(x, P, 1, keep, torch.bfloat16)
        bwd[f"patchify_keep_bwd {frac}"] = lambda dout=dout, slot=slot: ops.patchify_keep_bwd(dout, x.shape, P, 1, slot,
                                                                                              torch.bfloat16)
        fwd_bytes[f"patchify_keep {frac}"] = 2 * kept_bytes
        bwd_bytes[f"patchify_keep_bwd {frac}"] = kept_bytes + clip_bytes
        del rows, want, dx, back
    head = ["| variant | median us | min us | max us | bytes moved | TB/s | share of the 6.29 TB/s copy rate |", "|---|---|---|---|---|---|---|"]
    lines = ["Forward (keep fraction = k / n, tube rows):", ""] + head
    times = _alternate(fwd, rounds, seconds)
    lines += [_row(name, times[name], fwd_bytes[name]) for name in fwd]
    spread = max(times["patchify"]) - min(times["patchify"])
    lines += ["", f"Spread of the repeated `patchify` windows in this run (max - min over {rounds} rounds): {spread * 1e6:.2f} us.", "",
              "Adjoint (reads the kept rows, writes every pixel of the clip):", ""] + head
    times = _alternate(bwd, rounds, seconds)
    lines += [_row(name, times[name], bwd_bytes[name]) for name in bwd]
    del fwd, bwd, held
    return lines


def bench_small(rounds, seconds):
    from dvt_amd import ops
    b, t, n, d = 8, 32, 196, 512
    k = n // 2
    S = b * t
    g = torch.Generator().manual_seed(1130)
    keys = torch.randint(-2 ** 31, 2 ** 31 - 1, (b, n), generator=g, dtype=torch.int64).to(torch.int32).cuda()
    state = torch.tensor([1130, 0], dtype=torch.int64, device="cuda")
    keep, slot = ops.keep_select(keys, k, rows_per=t)
    emb = torch.randn(S * k, d, generator=g).to(torch.bfloat16).cuda()
    cls = torch.randn(d, generator=g).cuda()
    pos = torch.randn(t, n + 1, d, generator=g).cuda()
    dout = torch.randn(S, k + 1, d, generator=g).to(torch.bfloat16).cuda()
    full_emb = torch.randn(S * n, d, generator=g).to(torch.bfloat16).cuda()
    variants = {"keep_select [8, 196] k 98 x 32 rows": lambda: ops.keep_select(keys, k, rows_per=t),
                "keep_draw [8, 196] k 98 x 32 rows": lambda: ops.keep_draw(b, n, k, state, 0, rows_per=t),
                "tokens_assemble_keep_fwd [256, 99, 512]": lambda: ops.tokens_assemble_keep_fwd(emb, cls, pos, keep),
                "tokens_assemble_keep_bwd [256, 99, 512]": lambda: ops.tokens_assemble_keep_bwd(dout, t, n + 1, slot),
                "tokens_assemble_fwd [256, 197, 512] (no dropout)": lambda: ops.tokens_assemble_fwd(full_emb, cls, pos, S, t, n)}
    times = _alternate(variants, rounds, seconds)
    lines = ["| launch | median us | min us | max us |", "|---|---|---|---|"]
    for name, v in times.items():
        lines.append(f"| `{name}` | {statistics.median(v) * 1e6:.2f} | {min(v) * 1e6:.2f} | {max(v) * 1e6:.2f} |")
    del variants
    return lines


def bench_step(rounds, seconds):
    from dvt_amd import functional as F
    from dvt_amd import ops
    from dvt_amd.dp import FlatParameters
    from dvt_amd.graph import capture_step
    from dvt_amd.models.vit import ViViT
    cdt, image, T = torch.bfloat16, 224, 32
    g = torch.Generator().manual_seed(1130)
    x = torch.randn(8, T, 3, image, image, generator=g).to(cdt).cuda()
    y = (torch.rand(8, 19, generator=g) < 0.2).float().cuda()
    rng_state = F._rng.tensor(x.device)                   # the one state tensor every captured draw addresses
    steps, rows, peak, held = {}, {}, {}, []
    for p in (0.0, 0.5, 0.75):
        ops._ws.clear()                                   # grow-only scratch of whatever ran before
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        torch.manual_seed(1130)
        net = ViViT(image, 16, 19, T, dim=512, depth=4, heads=8, dim_head=64, compute_dtype=cdt, patch_dropout=p).cuda().train()
        flat = FlatParameters(net, compute_dtype=cdt)
        flat.sync_compute_copy()
        seed = torch.full((), flat.loss_scale, device="cuda")

        def step(net=net, flat=flat, seed=seed, x=x, y=y):
            flat.zero_grad()
            loss, _ = net.loss(x, y)
            loss.backward(seed)
            flat.finish_backward()
            F.next_step()                                 # device-side: the replayed graph draws a new subset every step
            return loss

        steps[p] = step
        held.append((net, flat, seed))
        rows[p] = 8 * T * (net.num_kept(net.num_patches) + 1)
        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        peak[p] = (torch.cuda.max_memory_allocated() - before) / 2 ** 30
    # one captured hipGraph per variant; the closures, the models behind them and the graphs' outputs are held in `steps`,
    # `held` and `captured` until every replay has finished
    captured = {p: capture_step(fn, warmup=1) for p, fn in steps.items()}
    times = _alternate({p: replay for p, (replay, _) in captured.items()}, rounds, seconds)
    torch.cuda.synchronize()
    assert F._rng.state is rng_state                      # nobody re-seeded between capture and the last replay
    base = statistics.median(times[0.0])
    lines = ["Launch form: hipGraph replay of zero_grad + forward + loss + backward + next_step (no optimizer step), metric shape "
             "b 8, T 32, 224^2, bf16, tube mode.", "",
             "| patch_dropout | ms / step | min | max | ratio to patch_dropout = 0 | space-stack rows | peak allocated GiB (model + step) |",
             "|---|---|---|---|---|---|---|"]
    for p in steps:
        med = statistics.median(times[p])
        lines.append(f"| {p} | {med * 1e3:.2f} | {min(times[p]) * 1e3:.2f} | {max(times[p]) * 1e3:.2f} | {med / base:.3f} | {rows[p]} | "
                     f"{peak[p]:.2f} |")
    del times, captured                                   # the graphs first, after the synchronize above ...
    del steps, held, x, y, rng_state                      # ... then what they addressed
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
        sys.exit("bench_patch_dropout: needs the MI355X; there is nothing to measure on a CPU")
    import dvt_amd
    dvt_amd._lib.load()
    dvt_amd.functional.manual_seed(1130)                  # once, before anything is built
    report = ["# Patch dropout: measurements", "", f"Device: {torch.cuda.get_device_name(0)}; windows of >= {args.window} s, "
              f"{args.rounds} alternating rounds, device events (`python tools/bench_patch_dropout.py --rounds {args.rounds} "
              f"--window {args.window}`).", "", "## Kept gather and adjoint: metric clip [8, 32, 3, 224, 224], bf16 -> bf16", ""]
    report += bench_gather(args.rounds, args.window)
    report += ["", "## The small launches, metric shape, keep fraction 0.5", ""]
    report += bench_small(max(3, args.rounds // 2), min(args.window, 0.2))
    if not args.skip_step:
        report += ["", "## Step: ViViT.loss forward + backward", ""]
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
