"""The device-side training augmentations at the frame loader's sizes on the MI355X (MMX_Frame_dl.py:63-71, :81-88), timed
with hipEvents (warm-up, then the median over the timed iterations).  One JSON line on stdout.

    python tools/bench_augment.py [--warmup 10] [--steps 50] [--pillow-repeats 3]
    rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/bench_augment.py --steps 20 --no-pillow
    python tools/bench_augment.py --kernel-trace DIR        # per-kernel medians of that trace, no GPU work

Work: B = 2 samples of 14 scenes -> 28 images, each a random resized crop of a 360 x 640 frame to 224 x 224 (table drawn by
input_stage.train_transform, seed 0), bf16 out; and 2 x 14 x 12 = 336 video frames of 112 x 112 bf16, erased in place with
the table of input_stage.RandomErasing (seed 0).  Timed on the same GPU and frames:
  augment      ops.frames_augment: the coefficient launch + the fused band launch (event-timed together; --kernel-trace
               splits them by kernel name)
  erase        ops.frames_erase: one launch
  preprocess   the unchanged ops.frames_preprocess, Resize(230) + CenterCrop(224), on the 28 frames: four launches and a
               uint8 intermediate in HBM, a comparable byte volume
  pillow       crop + resize + transpose + normalise of the same 28 images through Pillow / numpy on one host thread
  floor_*      bytes that must move / HBM peak: augment reads each sample's window once (3 h w bytes) and writes the output;
               the coefficient launch writes its tables; erase writes the rectangles; preprocess reads the frames, writes
               and rereads the intermediate [F, H0, 224, 3] and writes the output
"""
from __future__ import annotations

import argparse
import csv
import glob
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
B, SCENES, CLIP, H0, W0, IMG, VID = 2, 14, 12, 360, 640, 224, 112
KERNELS = ("augment_coeff_kernel", "augment_band_kernel", "erase_kernel", "resample_coeff_kernel", "resample_h_kernel",
           "resample_v_norm_kernel")


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


def kernel_trace(directory):
    """Median / count of the durations (us) of this stage's kernels in a rocprofv3 kernel-trace CSV under ``directory``."""
    files = glob.glob(os.path.join(directory, "**", "*kernel_trace.csv"), recursive=True)
    if not files:
        raise SystemExit(f"no *kernel_trace.csv under {directory}")
    dur = {k: [] for k in KERNELS}
    for r in csv.DictReader(open(files[0])):
        for k in KERNELS:
            if k in r["Kernel_Name"]:                 # mangled or demangled: the names do not contain one another
                dur[k].append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    return {k: {"median_us": round(float(np.median(v)), 2), "n": len(v)} for k, v in dur.items() if v}


def _pillow(frames, table, mean, std, repeats):
    from PIL import Image
    mean32, std32 = np.asarray(mean, np.float32).reshape(3, 1, 1), np.asarray(std, np.float32).reshape(3, 1, 1)
    best = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for f, top, left, h, w, hf, vf in table:
            img = Image.fromarray(frames[f]).crop((left, top, left + w, top + h)).resize((IMG, IMG), Image.BILINEAR)
            img = img.transpose(Image.FLIP_LEFT_RIGHT) if hf else img
            img = img.transpose(Image.FLIP_TOP_BOTTOM) if vf else img
            _ = (np.asarray(img).astype(np.float32).transpose(2, 0, 1) / np.float32(255) - mean32) / std32
        best.append((time.perf_counter() - t0) * 1e3)
    return {"median_ms": round(float(np.median(best)), 2), "repeats": repeats, "threads": 1}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--pillow-repeats", type=int, default=3)
    ap.add_argument("--no-pillow", action="store_true")
    ap.add_argument("--kernel-trace", metavar="DIR", help="summarise a rocprofv3 kernel trace instead of timing")
    a = ap.parse_args()
    if a.kernel_trace:
        print(json.dumps({"kernel_trace": kernel_trace(a.kernel_trace)}))
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench_augment.py times the MI355X: no GPU visible, nothing measured")
    from dvt_amd import input_stage as S
    from dvt_amd import ops

    N, F = B * SCENES, B * SCENES * CLIP
    rng = np.random.default_rng(0)
    frames = rng.integers(0, 256, (N, H0, W0, 3), dtype=np.uint8)
    dev = torch.from_numpy(frames).cuda()
    tt = S.train_transform(torch.bfloat16, generator=torch.Generator().manual_seed(0))
    table = tt.draw(H0, W0, range(N))
    out = tt(dev, params=table)
    assert out.shape == (N, 3, IMG, IMG)
    clip = torch.randn(F, 3, VID, VID, device="cuda").to(torch.bfloat16)
    er = S.RandomErasing(generator=torch.Generator().manual_seed(0))
    etab = er.draw(VID, VID, F)

    res = {"shape": dict(images=N, frame=[H0, W0], out=IMG, erase_frames=F, erase_hw=VID), "warmup": a.warmup, "steps": a.steps}
    res["augment"] = _stats(_time(lambda: ops.frames_augment(dev, table, (IMG, IMG), tt.mean, tt.std, torch.bfloat16),
                                  a.warmup, a.steps))
    res["erase"] = _stats(_time(lambda: ops.frames_erase(clip, etab), a.warmup, a.steps))
    res["preprocess"] = _stats(_time(lambda: ops.frames_preprocess(dev, 230, IMG, tt.mean, tt.std, torch.bfloat16),
                                     a.warmup, a.steps))
    if not a.no_pillow:
        res["pillow"] = _pillow(frames, table.tolist(), tt.mean, tt.std, a.pillow_repeats)

    t = table.numpy().astype(np.int64)
    window = int((3 * t[:, 3] * t[:, 4]).sum())
    ks_w, ks_h = int(np.ceil(max(W0 / IMG, 1.0))) * 2 + 1, int(np.ceil(max(H0 / IMG, 1.0))) * 2 + 1
    e = etab.numpy().astype(np.int64)
    resized_w = int(230 * W0 / H0)
    byts = {
        "floor_augment_bands": window + N * 3 * IMG * IMG * 2,
        "floor_augment_coeff": 4 * N * (8 + IMG * (2 + ks_w) + IMG * (2 + ks_h)),
        "floor_erase": int((e[:, 2] * e[:, 3]).sum()) * 3 * 2,
        "floor_preprocess": N * H0 * W0 * 3 + 2 * N * H0 * IMG * 3 + N * 3 * IMG * IMG * 2 + 4 * (resized_w * (2 + ks_w) + 230 * (2 + ks_h)),
    }
    for k, v in byts.items():
        res[k] = {"bytes": v, "us": round(v / (HBM_PEAK_GBS * 1e9) * 1e6, 3)}
    res["erased_frames"] = int((e[:, 2] != 0).sum())
    print(json.dumps(res))


if __name__ == "__main__":
    main()
