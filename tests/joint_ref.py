"""Float64 CPU statement of joint space-time attention (models.JointViViT), pinned to the imported reference modules by
tests/golden/joint_vivit.npz (tools/gen_golden_joint.py).  It builds on oracle/clip_path.py (the pre-norm Transformer, the
LayerNorm, the loss) and tests/tubelet_ref.py (the gather) and runs autograd in the dtype of its inputs.

  tokens of clip bi: [CLS] + the t' n rows of the tubelet gather in (tau, h, w) order, plus one positional row each.
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from oracle import clip_path as O
from tests import tubelet_ref as TR
from tests.util import digest_idx

Tensor = torch.Tensor
VARIANTS = {"cls_t1": ("cls", 1), "mean_t1": ("mean", 1), "cls_t2": ("cls", 2)}


def forward(x: Tensor, P: Dict[str, Tensor], *, patch: int, depth: int, heads: int, pool: str, pt: int = 1) -> Tensor:
    """clip [b, t, C, H, W] and the state dict of a ``JointViViT`` -> logits [b, classes]"""
    b = x.shape[0]
    rows = TR.gather(x, patch, pt)                                              # [b t' n, pt P P C]
    emb = O.linear(rows, P["to_patch_embedding.1.weight"], P["to_patch_embedding.1.bias"])
    d = emb.shape[-1]
    emb = emb.reshape(b, -1, d)
    tok = torch.cat((P["cls_token"].reshape(1, 1, d).expand(b, 1, d), emb), dim=1)
    tok = tok + P["pos_embedding"].reshape(1, -1, d)[:, :tok.shape[1]]
    z = O.prenorm_transformer(tok, P, "transformer.", depth, heads)
    pooled = z.mean(dim=1) if pool == "mean" else z[:, 0]
    h = O.layernorm(pooled, P["mlp_head.0.weight"], P["mlp_head.0.bias"])
    return O.linear(h, P["mlp_head.1.weight"], P["mlp_head.1.bias"])


def step(x: Tensor, P: Dict[str, Tensor], target: Tensor, **kw):
    """(logits, loss, {name: gradient}) -- every parameter's and, under "clip", the clip's"""
    leaves = {name: v.detach().clone().requires_grad_(True) for name, v in P.items()}
    xl = x.detach().clone().requires_grad_(True)
    logits = forward(xl, leaves, **kw)
    loss = O.bce_with_logits(logits, target.to(logits.dtype))
    grads = torch.autograd.grad(loss, list(leaves.values()) + [xl])
    out = dict(zip(leaves, grads[:-1]))
    out["clip"] = grads[-1]
    return logits.detach(), loss.detach(), out


def config(npz):
    return {k[4:]: int(npz[k]) for k in npz.files if k.startswith("cfg_")}


def inputs(npz):
    """(clip f32, target f32) of the fixture: the clip regenerated from its seed"""
    cfg = config(npz)
    rng = np.random.default_rng(int(npz["x_seed"]))
    clip = rng.standard_normal((int(npz["batch"]), cfg["frames"], 3, cfg["image"], cfg["image"])).astype(np.float32)
    return torch.from_numpy(clip), torch.from_numpy(npz["target"])


def deviations(npz, tag: str, logits: Tensor, loss, grads: Dict[str, Tensor]) -> Dict[str, float]:
    """The generator's measures of a run against the float64 result stored under ``tag``: "logits" rel-L2, "loss" relative,
    "g:<name>" the larger of the rel-L2 error on the digest entries and the relative error of the L2 norm."""
    rl = torch.from_numpy(npz[f"{tag}:logits"])
    rs = float(npz[f"{tag}:loss"])
    out = {"logits": float((logits.detach().double().cpu() - rl).norm() / rl.norm()),
           "loss": abs(float(loss) - rs) / abs(rs)}
    pre = f"{tag}:gs:"
    for key in npz.files:
        if not key.startswith(pre):
            continue
        name = key[len(pre):]
        s, n = torch.from_numpy(npz[key]), float(npz[f"{tag}:gn:{name}"])
        g = grads[name].detach().double().cpu()
        flat = g.reshape(-1)
        got = flat[torch.from_numpy(digest_idx(tuple(g.shape)))]
        out["g:" + name] = max(float((got - s).norm() / (s.norm() + 1e-30)), abs(float(flat.norm()) - n) / (n + 1e-30))
    return out
