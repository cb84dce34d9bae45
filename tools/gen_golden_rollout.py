#!/usr/bin/env python3
"""Writes tests/golden/attention_rollout.npz: attention rollout of the IMPORTED reference ViViT (build container only; the
reference is loaded by file path and nothing of it is copied).

Every ``to_qkv`` of the reference model (src/models/vit.py:39,48) is hooked, one seeded clip runs through it, and the
float64 restatement tests/rollout_ref.py turns the hooked Q and K into r_space, r_time and the video volume.  Stored: the
clip, what regenerates the weights, the hooked to_qkv outputs (so that the CPU test can redo the restatement without the
reference), the three float64 results, and the reference's OWN bf16 / fp16 deviations -- the same
rollout with the model and the clip cast to that type on the CPU, rel-L2 per output -- which the GPU tests hold the 16-bit
kernels to a multiple of, as the ``*_lowprec`` fixtures do.

Weights: 413,509 parameters do not fit a committed fixture next to the clip, so they are not stored; like the large ViViT
fixtures they come from ``tests.util.fill_state_from_numpy`` (numpy PCG64, platform independent) with seed ``fill_seed``,
after which every ``to_qkv.weight`` is multiplied by ``qkv_gain``: with an unscaled fill the attention is nearly uniform and
a wrong key order would move the answer by a few per cent only.  The generator asserts that the fixture can tell:
  (a) per-frame patch max / min of r_space >= 5;
  (b) the rollout with every layer's keys rotated by one differs from the right one by >= 0.1 x its maximum;
  (c) max |scale q . k| <= 20 (the exponent range the kernel tests' bound is derived for).

    python tools/gen_golden_rollout.py
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import rollout_ref as R                        # noqa: E402
from tests.util import fill_state_from_numpy              # noqa: E402

REF = "/root/reference/src/models/vit.py"
OUT = os.path.join(ROOT, "tests", "golden", "attention_rollout.npz")
SEED = 1130                                               # src/main.py:25
CFG = dict(image=32, patch=8, classes=5, frames=3, dim=64, depth=3, heads=2, dim_head=64)
BATCH = 2
QKV_GAIN = 5.0
RHO = 0.5


def build(vit, dtype=torch.float32):
    net = vit.ViViT(CFG["image"], CFG["patch"], CFG["classes"], CFG["frames"], dim=CFG["dim"], depth=CFG["depth"],
                    heads=CFG["heads"], dim_head=CFG["dim_head"]).eval()
    fill_state_from_numpy(net.named_parameters(), SEED + 1)
    with torch.no_grad():
        for name, p in net.named_parameters():
            if name.endswith("to_qkv.weight"):
                p.mul_(QKV_GAIN)
    return net.to(dtype)


def run(net, clip):
    space, time, handles = R.hook_to_qkv(net)
    with torch.no_grad():
        net(clip)
    for h in handles:
        h.remove()
    return space, time


def main() -> None:
    spec = importlib.util.spec_from_file_location("ref_vit", REF)
    vit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vit)
    torch.manual_seed(SEED)
    rng = np.random.default_rng(SEED + 2)
    clip = torch.from_numpy(rng.standard_normal((BATCH, CFG["frames"], 3, CFG["image"], CFG["image"])).astype(np.float32))
    net = build(vit)
    space, time = run(net, clip)
    r_space, r_time, video = R.vivit_rollout(space, time, CFG["heads"], RHO)
    ratio, diff, smax = R.fixture_conditions(r_space, space, time, CFG["heads"], RHO)
    print(f"(a) patch max/min >= {ratio:.2f}   (b) rotated keys differ by >= {diff:.3f} x max   (c) max |s| = {smax:.2f}")
    assert ratio >= 5.0 and diff >= 0.1 and smax <= 20.0, "the fixture would not tell a wrong kernel from a right one"
    out = {"clip": clip.numpy(), "fill_seed": np.array(SEED + 1), "qkv_gain": np.array(QKV_GAIN), "rho": np.array(RHO),
           "r_space": r_space.numpy(), "r_time": r_time.numpy(), "video": video.numpy(),
           "qkv_space": torch.stack(space).numpy(), "qkv_time": torch.stack(time).numpy()}   # the hooked to_qkv outputs, f32
    for k, v in CFG.items():
        out["cfg_" + k] = np.array(v)
    for tag, dtype in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
        sp, tm = run(build(vit, dtype), clip.to(dtype))
        lo = R.vivit_rollout(sp, tm, CFG["heads"], RHO)
        for name, a, b in zip(("r_space", "r_time", "video"), lo, (r_space, r_time, video)):
            out[f"{tag}:{name}_err"] = np.array(R.rel_l2(a, b))
        print(tag, [float(out[f"{tag}:{n}_err"]) for n in ("r_space", "r_time", "video")])
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
