#!/usr/bin/env python3
"""Writes tests/golden/drop_path.npz: the IMPORTED reference ViViT, in float64, with stochastic depth on fixed keep sets
(build container only; the reference is loaded by file path and nothing of it is copied).

The reference has no drop path, so its ``forward`` (src/models/vit.py:109-128) is walked submodule by submodule in its own
order, and each residual line of ``Transformer.forward`` (:73-74) is run under the rule
``x = x + scatter(alpha * fn(x[keep]))``: the reference's own ``PreNorm(Attention)`` / ``PreNorm(FeedForward)`` module is
called on the kept sequences only and its output added back into those rows.  Every module that computes is the reference's.

Three cases share the clip, the targets, the weights and the keep sets: ``subset`` (alpha = S / k), ``bernoulli``
(alpha = 1 / (1 - p_l) at drop_path = 0.3) and ``combined`` (``subset`` with the space stack on a kept subset of the patch
tokens).  Stored: what regenerates the clip (``x_seed``) and the weights (``tests.util.fill_state_from_numpy`` with
``fill_seed``), the targets, the keep sets, and per case the logits, the BCE loss and a digest of every gradient
(``tests.util.digest_idx`` entries and the L2 norm, float64).  tests/test_drop_path_cpu.py holds tests/droppath_ref.py to it.

    python tools/gen_golden_drop_path.py
"""
from __future__ import annotations

import importlib.util
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.util import digest_idx, fill_state_from_numpy              # noqa: E402
from tests import droppath_ref as DR                                  # noqa: E402  (index rules only: alphas)

REF = "/root/reference/src/models/vit.py"
OUT = os.path.join(ROOT, "tests", "golden", "drop_path.npz")
SEED = 1130                                               # src/main.py:25
CFG = dict(image=32, patch=8, classes=19, frames=4, dim=32, depth=2, heads=2, dim_head=16)
BATCH = 3                                                 # S = 12 in the space stack, S = 3 in the temporal stack
DROP_PATH = 0.3
PATCH_KEPT = 5                                            # of n = 16 positions (the combined case)


def stack(tr, x, keeps, scales):
    """Transformer.forward (vit.py:71-75) with each residual line on its kept sequences."""
    for i, (attn, ff) in enumerate(tr.layers):
        for j, fn in ((2 * i, attn), (2 * i + 1, ff)):
            if keeps[j] is None:
                x = fn(x) + x                                                      # :73-74 as written
            else:
                idx = keeps[j].long()
                x = x.index_add(0, idx, scales[j] * fn(x[idx]))
    return tr.norm(x)


def forward(net, clip, keeps, scales, patch_keep=None):
    depth = len(net.space_transformer.layers)
    x = net.to_patch_embedding(clip)                                               # vit.py:110
    b, t, n, d = x.shape
    x = torch.cat((net.space_token.reshape(1, 1, 1, d).expand(b, t, 1, d), x), dim=2)   # :113-114
    x = x + net.pos_embedding[:, :, :(n + 1)]                                       # :115
    x = net.dropout(x)                                                              # :116
    x = x.reshape(b * t, n + 1, d)                                                  # :118
    if patch_keep is not None:
        rows = torch.cat((torch.zeros(b * t, 1, dtype=torch.int64), 1 + patch_keep.long()), dim=1)
        x = torch.stack([x[s, rows[s]] for s in range(b * t)])
    x = stack(net.space_transformer, x, keeps[:2 * depth], scales[:2 * depth])     # :119
    x = x[:, 0].reshape(b, t, d)                                                    # :120
    x = torch.cat((net.temporal_token.expand(b, 1, d), x), dim=1)                   # :122-123
    x = stack(net.temporal_transformer, x, keeps[2 * depth:], scales[2 * depth:])  # :125
    x = x.mean(dim=1) if net.pool == "mean" else x[:, 0]                            # :126
    return net.mlp_head(x)                                                          # :128


def main() -> None:
    spec = importlib.util.spec_from_file_location("ref_vit", REF)
    vit = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(vit)
    rng = np.random.default_rng(SEED + 5)
    x_seed = SEED + 6
    clip = torch.from_numpy(np.random.default_rng(x_seed).standard_normal(
        (BATCH, CFG["frames"], 3, CFG["image"], CFG["image"])).astype(np.float32)).double()
    target = torch.from_numpy((rng.random((BATCH, CFG["classes"])) < 0.3).astype(np.float64))
    S, St, depth = BATCH * CFG["frames"], BATCH, CFG["depth"]

    def pick(s, k):
        return torch.from_numpy(np.sort(rng.permutation(s)[:k]).astype(np.int32))

    # per branch, execution order: space (attn, ff) x depth, then temporal; among them a None, a k = 1 and a k = S
    keeps = [pick(S, 7), None, pick(S, 1), pick(S, S), pick(St, 2), pick(St, 1), None, pick(St, St)]
    n = (CFG["image"] // CFG["patch"]) ** 2
    patch_keep = torch.from_numpy(np.stack([np.sort(rng.permutation(n)[:PATCH_KEPT]) for _ in range(S)]).astype(np.int32))
    net = vit.ViViT(CFG["image"], CFG["patch"], CFG["classes"], CFG["frames"], dim=CFG["dim"], depth=depth,
                    heads=CFG["heads"], dim_head=CFG["dim_head"]).eval()
    fill_state_from_numpy(net.named_parameters(), SEED + 7)
    net = net.double()
    out = {"x_seed": np.array(x_seed), "batch": np.array(BATCH), "target": target.numpy(), "fill_seed": np.array(SEED + 7),
           "branches": np.array(len(keeps)), "drop_path": np.array(DROP_PATH), "patch_keep": patch_keep.numpy()}
    for j, e in enumerate(keeps):
        if e is not None:
            out[f"keep{j}"] = e.numpy()
    for k, v in CFG.items():
        out["cfg_" + k] = np.array(v)
    for case, mode, pk in (("subset", "subset", None), ("bernoulli", "bernoulli", None), ("combined", "subset", patch_keep)):
        scales = DR.alphas(keeps, S, St, depth, DROP_PATH, mode)
        net.zero_grad(set_to_none=True)
        logits = forward(net, clip, keeps, scales, pk)
        loss = torch.nn.BCEWithLogitsLoss()(logits, target)
        loss.backward()
        out[f"{case}:logits"] = logits.detach().numpy()
        out[f"{case}:loss"] = loss.detach().numpy()
        for name, p in net.named_parameters():
            g = p.grad.detach().reshape(-1)
            out[f"{case}:gs:{name}"] = g[torch.from_numpy(digest_idx(tuple(p.shape)))].numpy()
            out[f"{case}:gn:{name}"] = np.array(float(g.norm()))
        print(f"{case}: loss {float(loss.detach()):.6f}")
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
