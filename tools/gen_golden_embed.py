#!/usr/bin/env python3
"""Generate tests/golden/embed_resnet50.npz from the *imported reference* (build container only; the reference is loaded
by file path and never copied):

    python tools/gen_golden_embed.py

The image / location expert of the reference's EmbeddingExtractor is torchvision's resnet50 with ``fc = Identity()``: the
global average of x4.  The reference's own ``custom_resnet.resnet50`` (same tree, same state-dict keys) is run in eval mode
at 2 x 3 x 224^2 (the only size its fixed AvgPool2d(7) admits) with weights and running statistics from
tests/embed_fill.py's seed; the fixture stores the embedding, the parameter names in fill order, and the reference's own
bf16 / fp16 deviation (torch.autocast on the CPU, relative L2 of the embedding against its fp32 run) -- no weights.
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.embed_fill import RESNET50_SEED, fill_resnet50, resnet50_input  # noqa: E402

REF = "/root/reference/src/models/custom_resnet.py"
OUT = os.path.join(ROOT, "tests", "golden", "embed_resnet50.npz")


def main():
    spec = importlib.util.spec_from_file_location("ref_custom_resnet_embed", REF)
    cr = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cr)
    torch.manual_seed(0)
    net = cr.resnet50(pretrained=False).eval()
    fill_resnet50(net)
    x = resnet50_input()
    with torch.no_grad():
        emb = net(x)[-1].mean(dim=(2, 3))
        out = {"embed": emb.numpy(), "seed": np.array(RESNET50_SEED), "x_seed": np.array(RESNET50_SEED + 1),
               "shape": np.array(x.shape), "keys": np.array([n for n, _ in net.named_parameters()])}
        for tag, dt in (("bf16", torch.bfloat16), ("fp16", torch.float16)):
            with torch.autocast("cpu", dtype=dt):
                lp = net(x)[-1].float().mean(dim=(2, 3))
            out[f"{tag}:err"] = np.array(float((lp - emb).norm() / emb.norm()))
            print(f"embed_resnet50[{tag}]: reference autocast rel L2 {float(out[tag + ':err']):.3e}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: embed {tuple(emb.shape)}, |embed| {float(emb.norm()):.4f}")


if __name__ == "__main__":
    main()
