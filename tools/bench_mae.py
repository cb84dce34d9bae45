#!/usr/bin/env python3
"""Measure masked-autoencoder pre-training on the MI355X: the restore launches, the two loss launches, the prediction head
and the pre-training step.

    python tools/bench_mae.py [--out profiles/mae.md] [--rounds 5] [--window 0.3] [--skip-step]

Timing as in tools/bench_patch_dropout.py: device events around windows of at least ``--window`` seconds of back-to-back
calls, after a warm-up of every variant; the variants alternate within one process, round by round, and a variant's figure is
the median over the rounds of its window means.

1. Launches at the metric clip [8, 32, 3, 224, 224] in bf16 (P = 16, decoder width 384), ``tubelet_size`` 1 and 2, mask ratios
   0.75 and 0.9: ``ops.tokens_restore_fwd`` / ``_bwd`` and ``ops.mae_loss_fwd`` (both launches) / ``_bwd`` with the bytes
   each moves (the masked patches' clip bytes, not the whole clip), against the device copy rate of the same run
   (``ops.copy_`` of the clip), ``ops.patchify`` / ``ops.tubelet_patchify`` on the same clip and ``ops.patchify_keep`` at the
   matching keep fraction.
2. The prediction head ``decoder_pred`` (a [S n, 384] x [384, D] GEMM) on all rows against the dropped rows only: what
   gathering the dropped rows first would save (not part of this tree).
3. Step: ``MaskedClipAutoencoder.forward`` + backward at the metric shape (encoder dim 512, depth 4, 8 heads; decoder 384,
   depth 4, 6 heads; bf16), each replayed from a captured hipGraph (``F.next_step()`` inside: a new mask per replay), next
   to ``ViViT.loss`` at ``patch_dropout`` 0 and 0.75 in the same run.

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

B, T, IMAGE, P, DEC = 8, 32, 224, 16, 384
N = (IMAGE // P) ** 2
RATIOS = (0.75, 0.9)


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


def _kept(ratio):
    return N - int(ratio * N)


def _tube_keep(S, t, k, seed):
    from dvt_amd import ops
    state = torch.tensor([seed, 0], dtype=torch.int64, device="cuda")
    return ops.keep_draw(S // t, N, k, state, 0, rows_per=t)


def bench_launches(rounds, seconds):
    from dvt_amd import ops
    cdt = torch.bfloat16
    g = torch.Generator().manual_seed(1130)
    x = torch.randn(B, T, 3, IMAGE, IMAGE, generator=g).to(cdt).cuda()
    clip_bytes = x.numel() * x.element_size()
    dst = torch.empty_like(x)
    variants = {"copy_ of the clip (device copy rate)": lambda: ops.copy_(dst, x)}
    nbytes = {"copy_ of the clip (device copy rate)": 2 * clip_bytes}
    held = []
    for pt in (1, 2):
        t = T // pt
        S, D = B * t, pt * P * P * 3
        name = "patchify" if pt == 1 else "tubelet_patchify pt 2"
        variants[name] = (lambda: ops.patchify(x, P, cdt)) if pt == 1 else (lambda: ops.tubelet_patchify(x, P, 2, cdt))
        nbytes[name] = 2 * clip_bytes
        pos = torch.randn(t, N, DEC, generator=g).cuda()
        mask = torch.randn(DEC, generator=g).cuda()
        pred = torch.randn(S, N, D, generator=g).to(cdt).cuda()
        dout = torch.randn(S, N, DEC, generator=g).to(cdt).cuda()
        one = torch.ones(1, device="cuda")
        held.append((pos, mask, pred, dout, one))
        for ratio in RATIOS:
            k = _kept(ratio)
            keep, slot = _tube_keep(S, t, k, 7)
            y = torch.randn(S, 1 + k, DEC, generator=g).to(cdt).cuda()
            _, _, stats = ops.mae_loss_fwd(pred, x, slot, k, P, pt, True)
            held.append((keep, slot, y, stats))
            tag = f"pt {pt} ratio {ratio} (k {k})"
            masked = S * (N - k) * D
            variants[f"patchify_keep {tag}"] = lambda keep=keep, pt=pt: ops.patchify_keep(x, P, pt, keep, cdt)
            nbytes[f"patchify_keep {tag}"] = 2 * S * k * D * 2
            variants[f"tokens_restore_fwd {tag}"] = lambda y=y, mask=mask, pos=pos, slot=slot, k=k: ops.tokens_restore_fwd(
                y, mask, pos, slot, k, 1)
            nbytes[f"tokens_restore_fwd {tag}"] = (S * k * DEC + S * N * DEC) * 2 + (t * N * DEC + DEC) * 4 + S * N * 4
            variants[f"tokens_restore_bwd {tag}"] = lambda dout=dout, keep=keep, slot=slot, t=t: ops.tokens_restore_bwd(
                dout, keep, slot, t, 1)
            nbytes[f"tokens_restore_bwd {tag}"] = (S * N * DEC + S * (1 + k) * DEC) * 2 + 3 * t * N * DEC * 4 + S * N * 4
            variants[f"mae_loss_fwd {tag}"] = lambda pred=pred, slot=slot, k=k, pt=pt: ops.mae_loss_fwd(pred, x, slot, k, P, pt, True)
            nbytes[f"mae_loss_fwd {tag}"] = masked * 4 + S * N * 16
            variants[f"mae_loss_bwd {tag}"] = lambda pred=pred, slot=slot, k=k, pt=pt, stats=stats, one=one: ops.mae_loss_bwd(
                pred, x, slot, k, P, pt, stats, one)
            nbytes[f"mae_loss_bwd {tag}"] = masked * 4 + S * N * D * 2 + S * N * 12
    times = _alternate(variants, rounds, seconds)
    copy = nbytes["copy_ of the clip (device copy rate)"] / statistics.median(times["copy_ of the clip (device copy rate)"])
    lines = [f"Device copy rate in this run (`ops.copy_` of the clip, {2 * clip_bytes / 1e6:.1f} MB moved): {copy / 1e12:.2f} TB/s.",
             "", "| launch | median us | min us | max us | bytes moved | TB/s | share of the copy rate | us at the copy rate |",
             "|---|---|---|---|---|---|---|---|"]
    for name, v in times.items():
        med = statistics.median(v)
        lines.append(f"| `{name}` | {med * 1e6:.2f} | {min(v) * 1e6:.2f} | {max(v) * 1e6:.2f} | {nbytes[name]} | "
                     f"{nbytes[name] / med / 1e12:.2f} | {nbytes[name] / med / copy:.2f} | {nbytes[name] / copy * 1e6:.2f} |")
    del variants, held
    return lines


def bench_head(rounds, seconds):
    """decoder_pred forward on all S n rows against the S (n - k) dropped rows."""
    from dvt_amd import ops
    cdt = torch.bfloat16
    g = torch.Generator().manual_seed(1130)
    variants, flops = {}, {}
    held = []
    for pt in (1, 2):
        S, D = B * T // pt, pt * P * P * 3
        w = (torch.randn(D, DEC, generator=g) / DEC ** 0.5).to(cdt).cuda()
        bias = torch.zeros(D).cuda()
        for rows, what in [(S * N, "all rows")] + [(S * (N - _kept(r)), f"dropped rows, ratio {r}") for r in RATIOS]:
            xr = torch.randn(rows, DEC, generator=g).to(cdt).cuda()
            held.append((xr, w, bias))
            name = f"decoder_pred pt {pt}: [{rows}, {DEC}] x [{DEC}, {D}] ({what})"
            variants[name] = lambda xr=xr, w=w, bias=bias: ops.linear_fwd(xr, w, bias)
            flops[name] = 2 * rows * DEC * D
    times = _alternate(variants, rounds, seconds)
    lines = ["| forward GEMM | median us | min us | max us | GFLOP | TFLOP/s |", "|---|---|---|---|---|---|"]
    for name, v in times.items():
        med = statistics.median(v)
        lines.append(f"| `{name}` | {med * 1e6:.2f} | {min(v) * 1e6:.2f} | {max(v) * 1e6:.2f} | {flops[name] / 1e9:.2f} | "
                     f"{flops[name] / med / 1e12:.1f} |")
    del variants, held
    return lines


def bench_step(rounds, seconds):
    from dvt_amd import functional as F
    from dvt_amd import ops
    from dvt_amd.dp import FlatParameters
    from dvt_amd.graph import capture_step
    from dvt_amd.models import MaskedClipAutoencoder
    from dvt_amd.models.vit import ViViT
    cdt = torch.bfloat16
    g = torch.Generator().manual_seed(1130)
    x = torch.randn(B, T, 3, IMAGE, IMAGE, generator=g).to(cdt).cuda()
    y = (torch.rand(B, 19, generator=g) < 0.2).float().cuda()
    rng_state = F._rng.tensor(x.device)                   # the one state tensor every captured draw addresses
    steps, rows, peak, held = {}, {}, {}, []
    configs = [("ViViT.loss patch_dropout 0", None, 1, 0.0), ("ViViT.loss patch_dropout 0.75", None, 1, 0.75)]
    configs += [(f"MAE tubelet_size {pt} mask_ratio {r}", "mae", pt, r) for pt in (1, 2) for r in RATIOS]
    for name, kind, pt, ratio in configs:
        ops._ws.clear()                                   # grow-only scratch of whatever ran before
        torch.cuda.empty_cache()
        before = torch.cuda.memory_allocated()
        torch.manual_seed(1130)
        enc = ViViT(IMAGE, P, 19, T, dim=512, depth=4, heads=8, dim_head=64, compute_dtype=cdt, tubelet_size=pt,
                    patch_dropout=0.0 if kind else ratio)
        net = (MaskedClipAutoencoder(enc, mask_ratio=ratio) if kind else enc).cuda().train()
        flat = FlatParameters(net, compute_dtype=cdt)
        flat.sync_compute_copy()
        seed = torch.full((), flat.loss_scale, device="cuda")

        def step(net=net, flat=flat, seed=seed, x=x, y=y, kind=kind):
            flat.zero_grad()
            loss = net(x)[0] if kind else net.loss(x, y)[0]
            loss.backward(seed)
            flat.finish_backward()
            F.next_step()                                 # device-side: the replayed graph draws a new mask every step
            return loss

        steps[name] = step
        held.append((net, flat, seed))
        k = (net.num_kept(N) if kind else enc.num_kept(N))
        rows[name] = f"{B * T // pt * (k + 1)}" + (f" / {B * T // pt * N}" if kind else "")
        step()
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        step()
        torch.cuda.synchronize()
        peak[name] = (torch.cuda.max_memory_allocated() - before) / 2 ** 30
    captured = {name: capture_step(fn, warmup=1) for name, fn in steps.items()}
    times = _alternate({name: replay for name, (replay, _) in captured.items()}, rounds, seconds)
    torch.cuda.synchronize()
    assert F._rng.state is rng_state                      # nobody re-seeded between capture and the last replay
    base = statistics.median(times["ViViT.loss patch_dropout 0"])
    lines = ["Launch form: hipGraph replay of zero_grad + forward + loss + backward + next_step (no optimizer step), metric shape "
             "b 8, T 32, 224^2, bf16, tube masks; encoder dim 512, depth 4, 8 heads; decoder 384, depth 4, 6 heads.", "",
             "| step | ms / step | min | max | ratio to ViViT.loss, patch_dropout 0 | encoder rows / decoder rows | "
             "peak allocated GiB (model + step) |", "|---|---|---|---|---|---|---|"]
    for name in steps:
        med = statistics.median(times[name])
        lines.append(f"| {name} | {med * 1e3:.3f} | {min(times[name]) * 1e3:.3f} | {max(times[name]) * 1e3:.3f} | {med / base:.3f} | "
                     f"{rows[name]} | {peak[name]:.2f} |")
    del times, captured                                   # the graphs first, after the synchronize above ...
    del steps, held, x, y, rng_state                      # ... then what they addressed
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
        sys.exit("bench_mae: needs the MI355X; there is nothing to measure on a CPU")
    import dvt_amd
    dvt_amd._lib.load()
    dvt_amd.functional.manual_seed(1130)                  # once, before anything is built
    report = ["# Masked-autoencoder pre-training: measurements", "",
              f"Device: {torch.cuda.get_device_name(0)}; windows of >= {args.window} s, {args.rounds} alternating rounds, device "
              f"events (`python tools/bench_mae.py --rounds {args.rounds} --window {args.window}`).", "",
              "## Launches: metric clip [8, 32, 3, 224, 224], bf16, P 16, decoder width 384", ""]
    report += bench_launches(args.rounds, args.window)
    report += ["", "## The prediction head on all rows and on the dropped rows only", ""]
    report += bench_head(max(3, args.rounds // 2), min(args.window, 0.2))
    if not args.skip_step:
        report += ["", "## Step: forward + backward", ""]
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
