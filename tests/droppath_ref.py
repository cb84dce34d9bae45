"""CPU reference of stochastic depth on whole sequences (csrc/drop_path.hip, ``ViViT(drop_path=, drop_path_mode=)``), float64.

A stack holds S sequences.  A residual branch ``x = fn(x) + x`` (src/models/vit.py:73-74) with a keep set ``keep`` (k ascending
unique sequence indices) and a scale alpha becomes ``x = x + scatter(alpha * fn(x[keep]))``.  The pieces:

  * ``gather`` / ``scatter_add`` -- the two kernels as index expressions, rounding included (fp32 arithmetic, one rounding on
    the store) when asked for a 32- or 16-bit type; in float64 they are exact;
  * ``slots_of`` -- the inverse map of a keep set, -1 for a dropped sequence;
  * ``alphas`` -- the scale of every branch: S / k in ``"subset"`` mode, 1 / (1 - p_l) in ``"bernoulli"`` mode, p_l the
    linear schedule over the 2 * depth layers;
  * ``forward`` / ``step`` -- the oracle's ViViT with the rule on every branch.  It is written the way the device does NOT do
    it: the branch is evaluated on ALL sequences and multiplied by a 0 / alpha mask -- the sequences of a stack do not meet
    inside a branch, so that equals running it on the kept ones.  tests/golden/drop_path.npz (the imported reference's layers
    run on ``x[keep]``, tools/gen_golden_drop_path.py) pins it.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Sequence

import torch

from oracle import clip_path as O

Tensor = torch.Tensor


def slots_of(keep: Tensor, S: int) -> Tensor:
    slot = torch.full((S,), -1, dtype=torch.int64)
    slot[keep.long()] = torch.arange(keep.numel())
    return slot.to(torch.int32)


def gather(x: Tensor, idx: Tensor, alpha: float = 1.0) -> Tensor:
    """y[j] = alpha * x[idx[j]] where 0 <= idx[j] < S, zeros otherwise.  16- / 32-bit x: fp32 product, rounded once."""
    S = x.shape[0]
    idx = idx.long()
    live = (idx >= 0) & (idx < S)
    rows = x[idx.clamp(0, S - 1)]
    wide = torch.float64 if x.dtype == torch.float64 else torch.float32
    y = rows.to(wide) * torch.tensor(alpha, dtype=wide)
    y = torch.where(live.reshape((-1,) + (1,) * (x.dim() - 1)), y, torch.zeros((), dtype=wide))
    return y.to(x.dtype)


def scatter_add(res: Tensor, y: Tensor, slot: Tensor, alpha: float = 1.0) -> Tensor:
    """out[s] = res[s] + alpha * y[slot[s]] where 0 <= slot[s] < k, res[s] otherwise, in float64 (the exact value: what a
    fused multiply-add rounds once)."""
    k = y.shape[0]
    slot = slot.long()
    live = ((slot >= 0) & (slot < k)).reshape((-1,) + (1,) * (res.dim() - 1))
    add = y.double()[slot.clamp(0, k - 1)] * alpha
    return res.double() + torch.where(live, add, torch.zeros((), dtype=torch.float64))


def rates(depth: int, drop_path: float):
    """Per-layer rate over the 2 * depth layers in execution order, space stack first (timm's linspace rule)."""
    n = 2 * depth
    return [drop_path * i / (n - 1) if n > 1 else drop_path for i in range(n)]


def kept(S: int, p: float) -> int:
    return S - math.floor(p * S)


def alphas(drop_keep: Sequence[Optional[Tensor]], S_space: int, S_time: int, depth: int, drop_path: float, mode: str):
    """The scale of each of the 4 * depth branches (None where the entry is None)."""
    r = rates(depth, drop_path)
    out = []
    for j, e in enumerate(drop_keep):
        if e is None:
            out.append(None)
            continue
        stack, S = (0, S_space) if j < 2 * depth else (1, S_time)
        layer = stack * depth + (j - stack * 2 * depth) // 2
        out.append(S / e.numel() if mode == "subset" else 1.0 / (1.0 - r[layer]))
    return out


def _mask(keep: Optional[Tensor], alpha: Optional[float], S: int, like: Tensor) -> Tensor:
    m = torch.ones(S, dtype=like.dtype)
    if keep is not None:
        m = torch.zeros(S, dtype=like.dtype)
        m[keep.long()] = alpha
    return m[:, None, None]


def transformer(x: Tensor, P: Dict[str, Tensor], prefix: str, depth: int, heads: int, keeps, scales) -> Tensor:
    """``oracle.clip_path.prenorm_transformer`` with every branch multiplied by its 0 / alpha mask before the add."""
    S = x.shape[0]
    for i in range(depth):
        a, f = f"{prefix}layers.{i}.0.", f"{prefix}layers.{i}.1."
        y = O.self_attention(O.layernorm(x, P[a + "norm.weight"], P[a + "norm.bias"]), P[a + "fn.to_qkv.weight"],
                             P.get(a + "fn.to_out.0.weight"), P.get(a + "fn.to_out.0.bias"), heads)
        x = x + _mask(keeps[2 * i], scales[2 * i], S, x) * y
        y = O.feedforward(O.layernorm(x, P[f + "norm.weight"], P[f + "norm.bias"]), P[f + "fn.net.0.weight"],
                          P[f + "fn.net.0.bias"], P[f + "fn.net.3.weight"], P[f + "fn.net.3.bias"])
        x = x + _mask(keeps[2 * i + 1], scales[2 * i + 1], S, x) * y
    return O.layernorm(x, P[prefix + "norm.weight"], P[prefix + "norm.bias"])


def forward(x: Tensor, P: Dict[str, Tensor], drop_keep, scales, *, patch: int, depth: int, heads: int,
            patch_keep: Optional[Tensor] = None) -> Tensor:
    """``oracle.clip_path.vivit_forward`` under the rule; ``patch_keep`` [S, k]: the space stack on those patch tokens."""
    tok = O.vivit_tokens(x, P, patch)
    b, t, n1, d = tok.shape
    tok = tok.reshape(b * t, n1, d)
    if patch_keep is not None:
        rows = torch.cat((torch.zeros(b * t, 1, dtype=torch.int64), 1 + patch_keep.long()), dim=1)
        tok = tok.gather(1, rows[:, :, None].expand(b * t, rows.shape[1], d))
    nb = 2 * depth
    s = transformer(tok, P, "space_transformer.", depth, heads, drop_keep[:nb], scales[:nb])
    tcls = P["temporal_token"].reshape(1, 1, d).expand(b, 1, d)
    z = transformer(torch.cat((tcls, s[:, 0].reshape(b, t, d)), dim=1), P, "temporal_transformer.", depth, heads,
                    drop_keep[nb:], scales[nb:])
    h = O.layernorm(z[:, 0], P["mlp_head.0.weight"], P["mlp_head.0.bias"])
    return O.linear(h, P["mlp_head.1.weight"], P["mlp_head.1.bias"])


def step(x: Tensor, target: Tensor, P: Dict[str, Tensor], drop_keep, scales, **kw):
    """(logits, loss, {name: gradient}) of BCE-with-logits on ``forward``, in the dtype of ``P``."""
    leaves = {name: v.detach().clone().requires_grad_(True) for name, v in P.items()}
    logits = forward(x, leaves, drop_keep, scales, **kw)
    loss = O.bce_with_logits(logits, target)
    grads = torch.autograd.grad(loss, list(leaves.values()), allow_unused=True)
    return logits.detach(), loss.detach(), {name: (g if g is not None else torch.zeros_like(leaves[name]))
                                            for name, g in zip(leaves, grads)}


CASES = {"subset": ("subset", False), "bernoulli": ("bernoulli", False), "combined": ("subset", True)}


def fixture(npz):
    """-> (cfg, clip float64, target, drop_keep, patch_keep) of tests/golden/drop_path.npz (the clip from its numpy seed)."""
    import numpy as np
    cfg = {k[4:]: int(npz[k]) for k in npz.files if k.startswith("cfg_")}
    clip = np.random.default_rng(int(npz["x_seed"])).standard_normal(
        (int(npz["batch"]), cfg["frames"], 3, cfg["image"], cfg["image"])).astype(np.float32)
    return (cfg, torch.from_numpy(clip).double(), torch.from_numpy(npz["target"]), fixture_keeps(npz),
            torch.from_numpy(npz["patch_keep"]))


def digest_errors(npz, case: str, logits: Tensor, grads: Dict[str, Tensor]) -> Dict[str, float]:
    """name -> rel-L2 of ``logits`` and of every gradient's digest (its stored entries, and its norm) against ``case``."""
    from tests.util import digest_idx, rel_l2
    errs = {"logits": rel_l2(logits, torch.from_numpy(npz[f"{case}:logits"]))}
    pre = f"{case}:gs:"
    for key in npz.files:
        if not key.startswith(pre):
            continue
        name = key[len(pre):]
        g = grads[name].detach().double().cpu().reshape(-1)
        ref_s, ref_n = torch.from_numpy(npz[key]).double(), float(npz[f"{case}:gn:{name}"])
        e_s = rel_l2(g[torch.from_numpy(digest_idx(tuple(grads[name].shape)))], ref_s)
        errs[name] = max(e_s, abs(float(g.norm()) - ref_n) / (ref_n + 1e-30))
    return errs


def fixture_keeps(npz):
    """drop_keep of tests/golden/drop_path.npz: a list of None / int32 tensors, in branch order."""
    out = []
    for j in range(int(npz["branches"])):
        out.append(torch.from_numpy(npz[f"keep{j}"]) if f"keep{j}" in npz.files else None)
    return out
