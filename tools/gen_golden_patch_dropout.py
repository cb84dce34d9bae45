#!/usr/bin/env python3
"""Writes tests/golden/patch_dropout.npz: the IMPORTED reference ViViT, in float64, run on a kept subset of its patch tokens
(build container only; the reference is loaded by file path and nothing of it is copied).

The reference has no patch dropout, so its ``forward`` (src/models/vit.py:109-128) is walked submodule by submodule in its
own order -- to_patch_embedding, CLS concat, ``+= pos_embedding``, dropout, space_transformer, temporal CLS concat,
temporal_transformer, pooling, mlp_head -- and the rows ``[0] + 1 + keep[s]`` of every sequence are selected right after
the positional add: every module that computes is the reference's.  Stored: the clip, the targets, the kept set, what
regenerates the weights (``tests.util.fill_state_from_numpy`` with ``fill_seed``), the logits, the BCE loss and the
gradient of every parameter.  tests/test_patch_dropout_cpu.py holds tests/patchdrop_ref.py to it at <= 1e-9 rel-L2.

    python tools/gen_golden_patch_dropout.py
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.util import fill_state_from_numpy              # noqa: E402

REF = "/root/reference/src/models/vit.py"
OUT = os.path.join(ROOT, "tests", "golden", "patch_dropout.npz")
SEED = 1130                                               # src/main.py:25
CFG = dict(image=32, patch=8, classes=19, frames=4, dim=32, depth=1, heads=2, dim_head=16)
BATCH = 2
KEPT = 5                                                  # of n = 16 positions per frame


def masked_forward(net, clip, keep):
    x = net.to_patch_embedding(clip)                                               # vit.py:110
    b, t, n, d = x.shape
    x = torch.cat((net.space_token.reshape(1, 1, 1, d).expand(b, t, 1, d), x), dim=2)   # :113-114
    x = x + net.pos_embedding[:, :, :(n + 1)]                                       # :115
    x = net.dropout(x)                                                              # :116
    x = x.reshape(b * t, n + 1, d)                                                  # :118
    rows = torch.cat((torch.zeros(b * t, 1, dtype=torch.int64), 1 + keep.long()), dim=1)
    x = torch.stack([x[s, rows[s]] for s in range(b * t)])                          # the kept rows of every sequence
    x = net.space_transformer(x)                                                    # :119
    x = x[:, 0].reshape(b, t, d)                                                    # :120
    x = torch.cat((net.temporal_token.expand(b, 1, d), x), dim=1)                   # :122-123
    x = net.temporal_transformer(x)                                                 # :125
    x = x.mean(dim=1) if net.pool == "mean" else x[:, 0]                            # :126
    return net.mlp_head(x)                                                          # :128


def main() -> None:
    spec = importlib.util.spec_from_file_location("ref_vit", REF)
    vit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vit)
    rng = np.random.default_rng(SEED + 3)
    n = (CFG["image"] // CFG["patch"]) ** 2
    clip = torch.from_numpy(rng.standard_normal((BATCH, CFG["frames"], 3, CFG["image"], CFG["image"])))
    target = torch.from_numpy((rng.random((BATCH, CFG["classes"])) < 0.3).astype(np.float64))
    keep = np.stack([np.sort(rng.permutation(n)[:KEPT]) for _ in range(BATCH * CFG["frames"])]).astype(np.int32)
    net = vit.ViViT(CFG["image"], CFG["patch"], CFG["classes"], CFG["frames"], dim=CFG["dim"], depth=CFG["depth"],
                    heads=CFG["heads"], dim_head=CFG["dim_head"]).eval()
    fill_state_from_numpy(net.named_parameters(), SEED + 4)
    net = net.double()
    logits = masked_forward(net, clip, torch.from_numpy(keep))
    loss = torch.nn.BCEWithLogitsLoss()(logits, target)
    loss.backward()
    out = {"clip": clip.numpy(), "target": target.numpy(), "keep": keep, "fill_seed": np.array(SEED + 4),
           "logits": logits.detach().numpy(), "loss": loss.detach().numpy()}
    for k, v in CFG.items():
        out["cfg_" + k] = np.array(v)
    for name, p in net.named_parameters():
        out["g:" + name] = p.grad.numpy()
    # the fixture tells a wrong positional row from the right one: the kept rows are not the first KEPT
    assert not all((row == np.arange(KEPT)).all() for row in keep)
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes); loss {float(loss.detach()):.6f}")


if __name__ == "__main__":
    main()
