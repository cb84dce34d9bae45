#!/usr/bin/env python3
"""Test-step throughput of FrameTransformer(model="vid") on the MI355X (the reference's trainer.test, main.py:111):

  * one test step at the reference shape: B = 2 samples x (13 + 1 CLS) chunks of 12 x 112^2, 19 classes, in bf16 and fp32,
    under torch.inference_mode() (eval(); the folded route where it is the faster one, video_resnet.inference_route)
    and on the eval() + no_grad route; for the R(2+1)D-18 encoder alone (28 clips) also the folded route itself
    (VideoResNet.features_folded) and torch's own eval forward of the same modules (nn.Conv3d / nn.BatchNorm3d, MIOpen);
  * per stage (stem, layer1 .. layer4) of the encoder: the folded route against the eval() + no_grad route;
  * per launch of the folded route's encoder (one step, 28 clips), grouped by geometry: the kernel it takes, the other
    candidate where a layer-1 half has two (dvt_conv2p1d_l1 / dvt_conv3d_implicit), and torch's conv3d (MIOpen, NCDHW)
    of the same geometry.

Timed with hipEvents, median of --steps after --warmup.  One JSON line on stdout.

    python tools/bench_test_epoch.py [--warmup 3] [--steps 10] [--dtypes bf16,fp32] [--no-layers]
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

R21D_GFLOP_PER_CLIP = 62.0         # 2 flop per MAC over every convolution of R(2+1)D-18 at 12 x 112^2 (shape arithmetic)


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


class _TorchR21D(torch.nn.Module):
    """torch's own eval forward of the R(2+1)D tree (the module's nn.Conv3d / nn.BatchNorm3d, called as torch modules)."""

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


def _model(dt):
    from dvt_amd.models.frame_transformer import FrameTransformer
    torch.manual_seed(0)
    net = FrameTransformer(batch_size=2, seq_len=13, cls=1, model="vid", opt="adamW", learning_rate=5e-6,
                           weight_decay=0.09, momentum=0.005, compute_dtype=dt)
    bb = net.vid_model.backbone
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():                                   # non-trivial running statistics: folding is not a no-op
        for m in bb.modules():
            if isinstance(m, torch.nn.BatchNorm3d):
                m.running_mean.copy_(0.1 * torch.randn(m.num_features, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
    return net.cuda().eval()


def _layers(net, vid, warmup, steps, with_torch):
    """Record every F.conv3d_bn_act call of one folded-route encoder forward, then time each one alone."""
    from dvt_amd import functional as F
    from dvt_amd import ops
    bb = net.vid_model.backbone
    names = {id(m): n for n, m in bb.named_modules()}
    calls = []
    real = F.conv3d_bn_act

    def rec(x, conv, bn, geom, **kw):
        calls.append((x, conv, bn, geom, kw))
        return real(x, conv, bn, geom, **kw)

    F.conv3d_bn_act = rec
    try:
        with torch.inference_mode():
            bb.features_folded(vid)
    finally:
        F.conv3d_bn_act = real
    res = {}
    with torch.inference_mode():
        for x, conv, bn, geom, kw in calls:
            name = names[id(conv)]
            k, s, p = tuple(conv.kernel_size), tuple(conv.stride), tuple(conv.padding)
            N, T, H, W = geom
            key = f"{conv.in_channels}->{conv.out_channels} k{k} s{s} {T}x{H}x{W}"
            ms = _time(lambda: real(x, conv, bn, geom, **kw), warmup, steps)
            alt = None
            if kw.get("route", "implicit") == "l1" or ops.conv2p1d_l1_supported(x, geom, conv.out_channels, tuple(conv.kernel_size),
                                                                                 tuple(conv.stride), tuple(conv.padding)):
                other = "implicit" if kw.get("route") == "l1" else "l1"        # the other candidate of a layer-1 half
                alt = (other, _time(lambda: real(x, conv, bn, geom, **dict(kw, route=other)), warmup, steps))
            To, Ho, Wo = (T + 2 * p[0] - k[0]) // s[0] + 1, (H + 2 * p[1] - k[1]) // s[1] + 1, (W + 2 * p[2] - k[2]) // s[2] + 1
            gf = 2.0 * N * To * Ho * Wo * conv.out_channels * conv.in_channels * k[0] * k[1] * k[2] / 1e9
            r = res.setdefault(key, {"modules": [], "gflop": gf, "route": kw.get("route", "implicit"), "ms": ms,
                                     "tflops": gf / ms})
            if alt is not None:
                r[f"{alt[0]}_ms"] = alt[1]
            r["modules"].append(name)
            if with_torch and "torch_ms" not in r:
                xt = torch.randn(N, conv.in_channels, T, H, W, device="cuda", dtype=x.dtype)
                wt = conv.weight.detach().to(x.dtype)
                r["torch_ms"] = _time(lambda: TF.conv3d(xt, wt, stride=s, padding=p), warmup, steps)
    total = sum(r["ms"] * len(r["modules"]) for r in res.values())
    return {"per_geometry": res, "sum_ms": total}


def _stages(bb, clips, warmup, steps):
    """Per stage (stem, layer1 .. layer4) of the encoder: the folded route against the eval() + no_grad route of the
    training kernels, each stage timed alone on its own route's input map."""
    from dvt_amd import functional as F
    from dvt_amd.models import video_resnet as V
    dt = bb.compute_dtype
    N, _, T, H, W = clips.shape
    s0, b0, s3, b3 = bb.stem[0], bb.stem[1], bb.stem[3], bb.stem[4]
    k, st, pd = s0.kernel_size[1:], s0.stride[1:], s0.padding[1:]
    H1, W1 = (H + 2 * pd[0] - k[0]) // st[0] + 1, (W + 2 * pd[1] - k[1]) // st[1] + 1
    frames = clips.permute(0, 2, 1, 3, 4).contiguous().view(N * T, 3, H, W)

    def stem_train():
        y = F.conv_bn_act_raw(frames, s0.weight, b0, (N * T, 3, H, W, True), k, st, pd, relu=True, dtype=dt, cpad=V.CPAD)
        return V._temporal((y, N, T, H1, W1), s3, b3, True, dt)

    def stem_folded():
        return V._folded_pair((V._clip_ndhwc8(clips, dt), N, T, H, W), bb.stem, bb.stem[4], True, dt)

    def run(layer, fm, folded):
        for blk in layer:
            fm = blk.forward_folded(fm, dt) if folded else blk.forward_ndhwc(fm, dt)
        return fm

    out = {}
    for folded, ctx, stem in ((True, torch.inference_mode, stem_folded), (False, torch.no_grad, stem_train)):
        tag = "folded_ms" if folded else "no_grad_ms"
        with ctx():
            out.setdefault("stem", {})[tag] = _time(stem, warmup, steps)
            fm = stem()
            for i, layer in enumerate((bb.layer1, bb.layer2, bb.layer3, bb.layer4)):
                out.setdefault(f"layer{i + 1}", {})[tag] = _time(lambda: run(layer, fm, folded), warmup, steps)
                fm = run(layer, fm, folded)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--dtypes", default="bf16,fp32")
    ap.add_argument("--no-layers", action="store_true")
    ap.add_argument("--only-ours", action="store_true")
    args = ap.parse_args()
    out = {"tool": "bench_test_epoch", "device": torch.cuda.get_device_name(0), "warmup": args.warmup,
           "steps": args.steps, "shape": "B=2 x 14 chunks x 12 x 112^2, 19 classes"}
    torch.backends.cudnn.benchmark = False
    dts = {"bf16": torch.bfloat16, "fp32": torch.float32}
    for tag in args.dtypes.split(","):
        dt = dts[tag]
        net = _model(dt)
        g = torch.Generator().manual_seed(2)
        batch = ((torch.rand(2, 19, generator=g) < 0.3).float().cuda(), None,
                 torch.randn(2, 13, 12, 3, 112, 112, generator=g).cuda())

        def step():
            net.test_step(batch, 0)
            net.running_logits, net.running_labels = [], []

        def infer():
            with torch.inference_mode():
                step()

        def no_grad():
            with torch.no_grad():
                step()

        rec = {"inference_ms": _time(infer, args.warmup, args.steps), "no_grad_ms": _time(no_grad, args.warmup, args.steps)}
        rec["speedup_vs_no_grad"] = rec["no_grad_ms"] / rec["inference_ms"]
        # the encoder alone, on the 28 clips of the step
        bb = net.vid_model.backbone
        clips = torch.randn(28, 3, 12, 112, 112, generator=g).cuda()
        with torch.inference_mode():
            rec["encoder_inference_ms"] = _time(lambda: bb.features(clips), args.warmup, args.steps)
            rec["encoder_folded_ms"] = _time(lambda: bb.features_folded(clips), args.warmup, args.steps)
            a = bb.features_folded(clips).float()
        with torch.no_grad():
            rec["encoder_no_grad_ms"] = _time(lambda: bb.features(clips), args.warmup, args.steps)
            b = bb.features(clips).float()
        rec["encoder_rel_l2_folded_vs_no_grad"] = float((a - b).norm() / b.norm())
        rec["encoder_folded_tflops"] = R21D_GFLOP_PER_CLIP * 28 / rec["encoder_folded_ms"]
        if not args.only_ours:
            tnet = _TorchR21D(copy.deepcopy(bb)).to(dt)                # (a copy: the measured module stays as it is)
            with torch.inference_mode():
                xt = clips.to(dt)
                rec["encoder_torch_ms"] = _time(lambda: tnet(xt), args.warmup, args.steps)
                rec["encoder_rel_l2_folded_vs_torch"] = float((a - tnet(xt).float()).norm() / tnet(xt).float().norm())
        if not args.no_layers:
            rec["stages"] = _stages(bb, clips, args.warmup, args.steps)
            rec["layers"] = _layers(net, clips, args.warmup, args.steps, not args.only_ours)
        out[tag] = rec
        print(f"[bench_test_epoch] {tag}: {json.dumps({k: v for k, v in rec.items() if k != 'layers'})}", file=sys.stderr,
              flush=True)
        del net, bb
        torch.cuda.empty_cache()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
