"""Grad-CAM of the FrameTransformer at the reference default (B = 2 -> 28 chunks of 12 x 112^2, tap behind layer4[-1]) on
the MI355X, timed with hipEvents (warm-up, then the median over the timed iterations).  One JSON line on stdout.

    timeout -k 10 600 python tools/bench_cam.py [--warmup 3] [--steps 15] [--batch 2]

Per compute dtype (bf16, fp32):
  forward        the eval() forward alone, under torch.no_grad()
  explain        FrameTransformer.explain(vid): the tapped forward, the seed, the backward to the tap, the map, the upsample
  cam_launches   the three new launches alone (dvt_cam_seed, dvt_cam_map, dvt_cam_render) on the call's own logits, A and G
  cam_overlay    dvt_cam_render with uint8 frames: mask and JET overlay in one launch
  eager_post     the same post-processing (argmax + one-hot, weights, map, scaling, trilinear upsample) with torch's eager
                 operators on the same GPU and the same tensors, ALTERNATED with cam_launches in one timed loop
The gate: cam_launches is not slower than eager_post.  Every figure is a time of this process's own launches.
"""
from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

torch.set_num_threads(min(16, torch.get_num_threads()))


def _stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(round(f * (len(s) - 1))))]  # noqa: E731
    return {"median_us": round(q(0.5) * 1e3, 2), "p10_us": round(q(0.1) * 1e3, 2), "p90_us": round(q(0.9) * 1e3, 2), "n": len(s)}


def _time(fns, warmup, steps):
    """Time the callables of ``fns`` alternately -> one list of milliseconds per callable."""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    ev = [[(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in fns] for _ in range(steps)]
    for row in ev:
        for fn, (a, b) in zip(fns, row):
            a.record()
            fn()
            b.record()
    torch.cuda.synchronize()
    return [[row[i][0].elapsed_time(row[i][1]) for row in ev] for i in range(len(fns))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--steps", type=int, default=15)
    ap.add_argument("--batch", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_cam needs the MI355X: a timing on the CPU says nothing")
    from dvt_amd import cam, ops
    from dvt_amd.models.frame_transformer import FrameTransformer

    B = a.batch
    rng = np.random.default_rng(7)
    vid = torch.from_numpy(rng.standard_normal((B, 13, 12, 3, 112, 112)).astype(np.float32)).cuda()
    frames = torch.from_numpy(rng.integers(0, 256, (B * 14, 12, 112, 112, 3), dtype=np.uint8)).cuda()
    res = {"batch": B, "chunks": B * 14, "warmup": a.warmup, "steps": a.steps, "tap": "layer4.1"}
    for mode, dt in (("bf16", torch.bfloat16), ("fp32", torch.float32)):
        out = res[mode] = {}
        torch.manual_seed(1)
        net = FrameTransformer(batch_size=B, seq_len=13, cls=1, model="vid", opt="adamW", learning_rate=5e-6, weight_decay=0.09,
                               momentum=0.005, compute_dtype=dt).cuda().eval()
        bb = net.vid_model.backbone

        def forward():
            with torch.no_grad():
                return net(None, vid)

        t_fwd, t_exp = _time([forward, lambda: net.explain(vid)], a.warmup, a.steps)
        out["forward"], out["explain"] = _stats(t_fwd), _stats(t_exp)

        # the call's own tensors: logits, tapped activation, gradient
        g = cam.GradCAM(net, [bb.layer4[-1]])
        for p in net.parameters():
            p.requires_grad_(False)
        bb.cam_tap = g.tap
        logits = net(None, vid)
        y, N, T, H, W = bb.cam_tapped
        (grad,) = torch.autograd.grad(logits, y, ops.cam_seed(logits))
        bb.cam_tap = bb.cam_tapped = None
        logits, C = logits.detach(), y.shape[1]
        A, G = y.detach().view(N, T * H * W, C), grad.view(N, T * H * W, C)
        size = (12, 112, 112)

        def hip_post():
            ops.cam_seed(logits)
            scaled, _, _ = ops.cam_map(A, G, "gradcam")
            return ops.cam_render(scaled.view(N, T, H, W), size)[0]

        def eager_post():
            torch.nn.functional.one_hot(logits.argmax(1), logits.shape[1]).to(logits.dtype)
            w = G.float().mean(1)
            raw = torch.relu((A.float() * w[:, None, :]).sum(2))
            r = raw - raw.amin(1, keepdim=True)
            s = r / (1e-7 + r.amax(1, keepdim=True))
            return torch.nn.functional.interpolate(s.view(N, 1, T, H, W), size=size, mode="trilinear", align_corners=False)[:, 0]

        def overlay():
            scaled, _, _ = ops.cam_map(A, G, "gradcam")
            return ops.cam_render(scaled.view(N, T, H, W), size, frames=frames)

        t_hip, t_eager, t_over = _time([hip_post, eager_post, overlay], a.warmup, a.steps)
        out["cam_launches"], out["eager_post"], out["cam_overlay"] = _stats(t_hip), _stats(t_eager), _stats(t_over)
        out["max_abs_vs_eager"] = float((hip_post() - eager_post()).abs().max())
        out["gate_cam_not_slower_than_eager"] = out["cam_launches"]["median_us"] <= out["eager_post"]["median_us"]
        out["explain_over_forward"] = round(out["explain"]["median_us"] / out["forward"]["median_us"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
