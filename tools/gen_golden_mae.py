#!/usr/bin/env python3
"""Writes tests/golden/mae.npz: masked-autoencoder pre-training assembled from the IMPORTED reference modules, in float64
(build container only; the reference is loaded by file path and nothing of it is copied).

The reference has no masked autoencoder.  Its ``ViViT`` supplies the encoder modules -- to_patch_embedding (whose Rearrange
also states the pixel targets), space_token, pos_embedding, dropout, space_transformer, walked in the order of its
``forward`` (src/models/vit.py:109-119) with the rows ``[0] + 1 + keep[s]`` selected right after the positional add -- and its
``Transformer`` the decoder; the pieces in between (decoder_embed, mask token, decoder positional table, decoder_pred, the
masked mean squared error with MAE's per-patch normalised targets) are stated here with torch.  The container registers its
parameters under the names and in the order of ``dvt_amd.models.mae.MaskedClipAutoencoder``, so one
``tests.util.fill_state_from_numpy`` call with ``fill_seed`` regenerates the weights on either side.  Stored: the clip, the
kept set, and per ``norm_pix_loss`` setting the loss, the per-patch losses and the gradient of every parameter that has one.
tests/test_mae_cpu.py holds tests/mae_ref.py to it at <= 1e-9 rel-L2.

    python tools/gen_golden_mae.py
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch
from torch import nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.util import fill_state_from_numpy              # noqa: E402

REF = "/root/reference/src/models/vit.py"
OUT = os.path.join(ROOT, "tests", "golden", "mae.npz")
SEED = 1130                                               # src/main.py:25
CFG = dict(image=32, patch=8, classes=19, frames=4, dim=32, depth=1, heads=2, dim_head=16,
           dec_dim=32, dec_depth=1, dec_heads=2, dec_dim_head=16)
BATCH = 2
KEPT = 5                                                  # of n = 16 positions per frame
EPS = 1e-6


class Container(nn.Module):
    """Parameter names and registration order of MaskedClipAutoencoder; every module that computes is the reference's."""

    def __init__(self, vit):
        super().__init__()
        n = (CFG["image"] // CFG["patch"]) ** 2
        dd = CFG["dec_dim"]
        self.mask_token = nn.Parameter(torch.zeros(1, 1, dd))
        self.decoder_pos_embedding = nn.Parameter(torch.zeros(1, CFG["frames"], n, dd))
        self.encoder = vit.ViViT(CFG["image"], CFG["patch"], CFG["classes"], CFG["frames"], dim=CFG["dim"], depth=CFG["depth"],
                                 heads=CFG["heads"], dim_head=CFG["dim_head"])
        self.decoder_embed = nn.Linear(CFG["dim"], dd)
        self.decoder = vit.Transformer(dd, CFG["dec_depth"], CFG["dec_heads"], CFG["dec_dim_head"], dd * 4)
        self.decoder_pred = nn.Linear(dd, 3 * CFG["patch"] ** 2)

    def forward(self, clip, keep, norm_pix):
        net = self.encoder
        x = net.to_patch_embedding(clip)                                               # vit.py:110
        b, t, n, d = x.shape
        x = torch.cat((net.space_token.reshape(1, 1, 1, d).expand(b, t, 1, d), x), dim=2)   # :113-114
        x = x + net.pos_embedding[:, :, :(n + 1)]                                       # :115
        x = net.dropout(x)                                                              # :116
        x = x.reshape(b * t, n + 1, d)                                                  # :118
        rows = torch.cat((torch.zeros(b * t, 1, dtype=torch.int64), 1 + keep.long()), dim=1)
        x = torch.stack([x[s, rows[s]] for s in range(b * t)])                          # the kept rows of every sequence
        x = net.space_transformer(x)                                                    # :119, final norm included
        z = self.decoder_embed(x)
        full = []
        for s in range(b * t):
            seq = self.mask_token.reshape(1, -1).repeat(n, 1)
            seq[keep[s].long()] = z[s, 1:]                                              # the CLS row is left out
            full.append(seq + self.decoder_pos_embedding[0, s % t])
        pred = self.decoder_pred(self.decoder(torch.stack(full)))
        target = net.to_patch_embedding[0](clip).reshape(b * t, n, -1)                  # the reference's own Rearrange
        if norm_pix:
            target = (target - target.mean(-1, keepdim=True)) / (target.var(-1, keepdim=True) + EPS) ** 0.5
        dropped = torch.ones(b * t, n, dtype=clip.dtype)
        for s in range(b * t):
            dropped[s, keep[s].long()] = 0.0
        per = ((pred - target) ** 2).mean(-1) * dropped
        return per.sum() / dropped.sum(), per


def main() -> None:
    spec = importlib.util.spec_from_file_location("ref_vit", REF)
    vit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vit)
    rng = np.random.default_rng(SEED + 5)
    n = (CFG["image"] // CFG["patch"]) ** 2
    clip32 = rng.standard_normal((BATCH, CFG["frames"], 3, CFG["image"], CFG["image"])).astype(np.float32)
    keep = np.stack([np.sort(rng.permutation(n)[:KEPT]) for _ in range(BATCH * CFG["frames"])]).astype(np.int32)
    assert not all((row == np.arange(KEPT)).all() for row in keep)      # a wrong positional row would show
    net = Container(vit).eval()
    fill_state_from_numpy(net.named_parameters(), SEED + 6)
    net = net.double()
    clip = torch.from_numpy(clip32).double()
    out = {"clip": clip32, "keep": keep, "fill_seed": np.array(SEED + 6),
           "names": np.array([name for name, _ in net.named_parameters()])}
    for k, v in CFG.items():
        out["cfg_" + k] = np.array(v)
    for norm_pix in (True, False):
        tag = "norm" if norm_pix else "raw"
        net.zero_grad(set_to_none=True)
        loss, per = net(clip, torch.from_numpy(keep), norm_pix)
        loss.backward()
        out[f"{tag}:loss"] = loss.detach().numpy()
        out[f"{tag}:per_patch"] = per.detach().numpy()
        for name, p in net.named_parameters():
            if p.grad is not None:
                out[f"{tag}:g:{name}"] = p.grad.numpy().copy()
        print(f"norm_pix_loss={norm_pix}: loss {float(loss.detach()):.6f}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
