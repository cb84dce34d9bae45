#!/usr/bin/env python3
"""Expert-embedding throughput on the MI355X (the reference's EmbeddingExtractor nets, eval mode, no grad):

  * r3d_18 features, clips of 3 x 16 x 112^2, N = 8 in bf16 and fp32 and N = 1 in bf16 (clips/s);
  * ResNet-50 embed, batch 64 at 224^2, bf16 (frames/s);
  * the yardstick: torch's own eval-mode forward of the same nets (nn.Conv3d / nn.Conv2d on MIOpen) with the same
    weights on the same GPU, and the relative L2 difference of the outputs.

Timed with hipEvents, median of --steps after --warmup.  One JSON line on stdout.  Per-launch kernel times of
dvt_conv3d_implicit come from running this under ``rocprofv3 --kernel-trace --stats`` (--only-ours keeps torch's
kernels out of that trace).

    python tools/bench_embed.py [--warmup 3] [--steps 10] [--only-ours]
"""
from __future__ import annotations

import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as TF  # noqa: E402

R3D_GFLOP_PER_CLIP = 81.4          # 2 flop per MAC over every convolution of r3d_18 at 16 x 112^2


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
    s = sorted(a.elapsed_time(b) for a, b in ev)
    return s[len(s) // 2]


class _TorchR3D(torch.nn.Module):
    """torch's own eval forward of the r3d_18 tree (the module's nn.Conv3d / nn.BatchNorm3d, called as torch modules)."""

    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        n = self.net
        y = n.stem(x)
        for layer in (n.layer1, n.layer2, n.layer3, n.layer4):
            for blk in layer:
                r = y if blk.downsample is None else blk.downsample(y)
                y = torch.relu(blk.conv2(blk.conv1(y)) + r)
        return y.mean(dim=(2, 3, 4))


class _TorchR50(torch.nn.Module):
    def __init__(self, net):
        super().__init__()
        self.net = net

    def forward(self, x):
        n = self.net
        y = n.maxpool(torch.relu(n.bn1(n.conv1(x))))
        for layer in (n.layer1, n.layer2, n.layer3, n.layer4):
            for b in layer:
                r = y if b.downsample is None else b.downsample(y)
                o = torch.relu(b.bn1(b.conv1(y)))
                o = torch.relu(b.bn2(b.conv2(o)))
                y = torch.relu(b.bn3(b.conv3(o)) + r)
        return y.mean(dim=(2, 3))


# r3d_18 convolution geometries at 16 x 112^2: (name, Cin, T, H, W, Cout, k, stride, pad, count per clip)
LAYERS = [("stem", 3, 16, 112, 112, 64, (3, 7, 7), (1, 2, 2), (1, 3, 3), 1),
          ("layer1", 64, 16, 56, 56, 64, (3, 3, 3), (1, 1, 1), (1, 1, 1), 4),
          ("layer2_first", 64, 16, 56, 56, 128, (3, 3, 3), (2, 2, 2), (1, 1, 1), 1),
          ("layer2", 128, 8, 28, 28, 128, (3, 3, 3), (1, 1, 1), (1, 1, 1), 3),
          ("layer3_first", 128, 8, 28, 28, 256, (3, 3, 3), (2, 2, 2), (1, 1, 1), 1),
          ("layer3", 256, 4, 14, 14, 256, (3, 3, 3), (1, 1, 1), (1, 1, 1), 3),
          ("layer4_first", 256, 4, 14, 14, 512, (3, 3, 3), (2, 2, 2), (1, 1, 1), 1),
          ("layer4", 512, 2, 7, 7, 512, (3, 3, 3), (1, 1, 1), (1, 1, 1), 3)]


def _layers(N, dt, warmup, steps, with_torch):
    """Per geometry: one dvt_conv3d_implicit launch against torch's conv3d (NCDHW, MIOpen) on the same data."""
    from dvt_amd import ops
    res = {}
    for name, Cin, T, H, W, Cout, k, s, p, count in LAYERS:
        cp = (Cin + 7) // 8 * 8
        x = torch.randn(N, Cin, T, H, W, device="cuda", dtype=dt)
        w = torch.randn(Cout, Cin, *k, device="cuda") * 0.05
        xd = torch.zeros(N, T, H, W, cp, device="cuda", dtype=dt)
        xd[..., :Cin] = x.permute(0, 2, 3, 4, 1)
        xd = xd.view(-1, cp)
        geom = (N, T, H, W)
        K = ops.conv3d_implicit_k(xd, geom, Cout, k, s, p)
        wd = ops.conv3d_weight_pack(w, cp, K, dt)
        gf = 2.0 * N * Cout * Cin * k[0] * k[1] * k[2] * torch.Size(ops.conv3d_out(geom, k, s, p)).numel() / 1e9
        ms = _time(lambda: ops.conv3d_implicit(xd, wd, geom, Cout, k, s, p), warmup, steps)
        rec = {"gflop": gf, "ms": ms, "tflops": gf / ms, "count_per_clip": count}
        if with_torch:
            wt = w.to(dt)
            tms = _time(lambda: TF.conv3d(x, wt, stride=s, padding=p), warmup, steps)
            rec.update(torch_ms=tms, torch_tflops=gf / tms, speedup=tms / ms)
        res[name] = rec
    return res


def _rel(a, b):
    a, b = a.float(), b.float()
    return float((a - b).norm() / b.norm())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--only-ours", action="store_true")
    args = ap.parse_args()
    from dvt_amd.models.video_resnet import r3d_18
    from dvt_amd.models.custom_resnet import resnet50
    from tests.embed_fill import fill_video_net, fill_resnet50

    dev = torch.device("cuda:0")
    out = {"tool": "bench_embed", "device": torch.cuda.get_device_name(0), "warmup": args.warmup, "steps": args.steps}
    torch.backends.cudnn.benchmark = False
    g = torch.Generator().manual_seed(0)
    base = r3d_18(compute_dtype=torch.float32)
    fill_video_net(base, 18)
    with torch.no_grad():
        for name, N, dt in (("r3d18_n8_bf16", 8, torch.bfloat16), ("r3d18_n8_fp32", 8, torch.float32),
                            ("r3d18_n1_bf16", 1, torch.bfloat16)):
            net = copy.deepcopy(base).to(dev).eval()
            net.compute_dtype = dt
            x = torch.randn(N, 3, 16, 112, 112, generator=g).to(dev)
            ms = _time(lambda: net.features(x), args.warmup, args.steps)
            rec = {"ms": ms, "clips_per_s": N / ms * 1e3, "tflops": R3D_GFLOP_PER_CLIP * N / ms}
            if not args.only_ours:
                tnet = _TorchR3D(copy.deepcopy(base).to(dev).eval().to(dt))
                tms = _time(lambda: tnet(x.to(dt)), args.warmup, args.steps)
                rec.update(torch_ms=tms, torch_clips_per_s=N / tms * 1e3, speedup=tms / ms,
                           rel_l2_vs_torch=_rel(net.features(x), tnet(x.to(dt))))
            out[name] = rec
            print(f"[bench_embed] {name}: {json.dumps(rec)}", file=sys.stderr, flush=True)
            del net
        r50 = resnet50(compute_dtype=torch.bfloat16)
        fill_resnet50(r50)
        r50 = r50.to(dev).eval()
        x = torch.randn(64, 3, 224, 224, generator=g).to(dev)
        ms = _time(lambda: r50.embed(x), args.warmup, args.steps)
        rec = {"ms": ms, "frames_per_s": 64 / ms * 1e3}
        if not args.only_ours:
            t50 = _TorchR50(copy.deepcopy(r50).to(torch.bfloat16))
            tms = _time(lambda: t50(x.to(torch.bfloat16)), args.warmup, args.steps)
            rec.update(torch_ms=tms, torch_frames_per_s=64 / tms * 1e3, speedup=tms / ms,
                       rel_l2_vs_torch=_rel(r50.embed(x), t50(x.to(torch.bfloat16))))
        out["resnet50_b64_bf16"] = rec
        print(f"[bench_embed] resnet50_b64_bf16: {json.dumps(rec)}", file=sys.stderr, flush=True)
        for N in (8, 1):
            out[f"layers_n{N}_bf16"] = _layers(N, torch.bfloat16, args.warmup, args.steps, not args.only_ours)
            print(f"[bench_embed] layers_n{N}_bf16: {json.dumps(out[f'layers_n{N}_bf16'])}", file=sys.stderr, flush=True)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
