"""AutoAugment on the device at the frame loader's sizes on the MI355X (the AutoAugment stage of MMX_Frame_dl.py:63-71), timed
with hipEvents (warm-up, then the median over the timed iterations).  One JSON line on stdout.

    python tools/bench_autoaugment.py [--warmup 10] [--steps 50] [--pillow-repeats 3] [--no-pillow] [--no-pairs]

Work: B = 2 samples of 14 scenes -> 28 images of 224 x 224 uint8 (random resized crops of 360 x 640 frames, table drawn by
input_stage.train_transform_autoaugment, seed 0), bf16 out.  Timed on the same GPU and images:
  autoaugment  ops.frames_autoaugment on the 28 cropped images with the drawn policy table: one launch
  chain        crop + flips to uint8 (ops.frames_augment, two launches) -> AutoAugment: the reference's whole line
  identity     the launch with two Identity slots per sample: the cost of the trip through LDS alone
  pairs        the launch with all 28 samples taking one sub-policy of the ImageNet policy, both operations applied, for each
               of its distinct sub-policies: which pair is slowest
  pillow       the same operations on the same 28 images through Pillow on one host thread, with ToTensor / Normalize in numpy
  floor        bytes that must move / HBM peak: each image read once (3 H W bytes) and its output written once
"""
from __future__ import annotations

import argparse
import importlib.util
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK_GBS = 8000.0
B, SCENES, H0, W0, IMG = 2, 14, 360, 640, 224


def _stats(ms):
    s = sorted(ms)
    q = lambda f: s[min(len(s) - 1, int(round(f * (len(s) - 1))))]  # noqa: E731
    return {"median_us": round(q(0.5) * 1e3, 2), "p10_us": round(q(0.1) * 1e3, 2), "p90_us": round(q(0.9) * 1e3, 2), "n": len(s)}


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
    return [a.elapsed_time(b) for a, b in ev]


def _pillow(images, names, mags, mean, std, repeats):
    from PIL import Image
    spec = importlib.util.spec_from_file_location("gen_golden_autoaugment", os.path.join(ROOT, "tools", "gen_golden_autoaugment.py"))
    G = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(G)
    mean32, std32 = np.asarray(mean, np.float32).reshape(3, 1, 1), np.asarray(std, np.float32).reshape(3, 1, 1)
    times = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for img, ops_, ms in zip(images, names, mags):
            pil = Image.fromarray(img)
            for op, m in zip(ops_, ms):
                pil = G.pillow_op(pil, op, m)
            _ = (np.asarray(pil).astype(np.float32).transpose(2, 0, 1) / np.float32(255) - mean32) / std32
        times.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(times)), 2), "repeats": repeats, "threads": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--pillow-repeats", type=int, default=3)
    ap.add_argument("--no-pillow", action="store_true")
    ap.add_argument("--no-pairs", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_autoaugment.py times the MI355X: no GPU visible, nothing measured")
    from dvt_amd import input_stage as S
    from dvt_amd import ops

    N = B * SCENES
    rng = np.random.default_rng(0)
    frames = torch.from_numpy(rng.integers(0, 256, (N, H0, W0, 3), dtype=np.uint8)).cuda()
    tt = S.train_transform_autoaugment(torch.bfloat16, generator=torch.Generator().manual_seed(0))
    crop = tt.first.draw(H0, W0, range(N))
    # the policy draws, kept by name as well as as a table: Pillow replays the same operations
    g = tt.second.generator
    names, mags, rows = [], [], []
    for _ in range(N):
        pid = int(torch.randint(len(tt.second.policy), (1,), generator=g).item())
        probs, signs = torch.rand((2,), generator=g), torch.randint(2, (2,), generator=g)
        ops_, ms, slots = [], [], []
        for i, (op, p, mid) in enumerate(tt.second.policy[pid]):
            if probs[i] <= p:
                m = S.autoaugment_magnitude(op, mid, int(signs[i]), IMG, IMG)
                ops_.append(op); ms.append(m); slots.append(S.autoaugment_slot(op, m, IMG, IMG))
            else:
                slots.append([0] * 8)
        names.append(ops_); mags.append(ms); rows.append(slots)
    table = torch.tensor(rows, dtype=torch.int32)
    u8 = ops.frames_augment(frames, crop, (IMG, IMG), out_dtype=torch.uint8)
    out = tt(frames, params=crop, policy_params=table)
    assert out.shape == (N, 3, IMG, IMG) and out.dtype == torch.bfloat16

    mean, std = tt.second.mean, tt.second.std
    launch = lambda t: ops.frames_autoaugment(u8, t, mean, std, torch.bfloat16)  # noqa: E731
    res = {"shape": dict(images=N, frame=[H0, W0], out=IMG), "warmup": a.warmup, "steps": a.steps,
           "applied_ops": int((table[:, :, 0] != 0).sum())}
    res["autoaugment"] = _stats(_time(lambda: launch(table), a.warmup, a.steps))
    res["chain"] = _stats(_time(lambda: tt(frames, params=crop, policy_params=table), a.warmup, a.steps))
    res["identity"] = _stats(_time(lambda: launch(torch.zeros(N, 2, 8, dtype=torch.int32)), a.warmup, a.steps))
    if not a.no_pairs:
        pairs = {}
        for sub in dict.fromkeys(tt.second.policy):
            slots = [S.autoaugment_slot(op, S.autoaugment_magnitude(op, mid, 1, IMG, IMG), IMG, IMG) for op, _, mid in sub]
            t = torch.tensor([slots] * N, dtype=torch.int32)
            pairs[f"{sub[0][0]}+{sub[1][0]}"] = _stats(_time(lambda: launch(t), 3, max(10, a.steps // 5)))["median_us"]
        res["pairs_us"] = dict(sorted(pairs.items(), key=lambda kv: -kv[1]))
    if not a.no_pillow:
        res["pillow"] = _pillow(u8.cpu().numpy(), names, mags, mean, std, a.pillow_repeats)
    byts = N * IMG * IMG * 3 + N * 3 * IMG * IMG * 2
    res["floor"] = {"bytes": byts, "us": round(byts / (HBM_PEAK_GBS * 1e9) * 1e6, 3)}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
