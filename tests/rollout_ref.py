"""Float64 restatement of attention rollout (TEST INFRASTRUCTURE; the device code is csrc/attn_rollout.hip), written from
the definition of the issue text (Abnar & Zuidema, 2020):

    P_l^h = softmax(scale Q_l^h K_l^h^T)   A_l = mean_h P_l^h   Ahat_l = rho I + (1 - rho) A_l   R = Ahat_L ... Ahat_1
    r = r0^T R

It builds the full N x N matrices and multiplies them AS MATRICES, then takes the row: deliberately not the vector
recurrence the kernels use.  Everything is float64; torch is storage and matmul only."""
from __future__ import annotations

import numpy as np
import torch

from tests import cam_ref


def probs(q: torch.Tensor, k: torch.Tensor, scale: float) -> torch.Tensor:
    """q, k [S, H, N, dh] -> P [S, H, N, N] float64 (rows: queries)."""
    s = torch.einsum("shid,shjd->shij", q.double(), k.double()) * scale
    return torch.softmax(s, dim=-1)


def lse(q: torch.Tensor, k: torch.Tensor, scale: float) -> torch.Tensor:
    """log-sum-exp of the scaled scores [S, H, N], float64."""
    s = torch.einsum("shid,shjd->shij", q.double(), k.double()) * scale
    return torch.logsumexp(s, dim=-1)


def layer_matrix(q, k, scale: float, rho: float) -> torch.Tensor:
    """Ahat [S, N, N]."""
    A = probs(q, k, scale).mean(1)
    N = A.shape[-1]
    return rho * torch.eye(N, dtype=torch.float64) + (1.0 - rho) * A


def rollout_matrix(layers, rho: float) -> torch.Tensor:
    """layers: [(q, k, scale)] in execution order (layer 1 first) -> R = Ahat_L ... Ahat_1 [S, N, N]."""
    R = None
    for q, k, scale in layers:
        A = layer_matrix(q, k, scale, rho)
        R = A if R is None else A @ R
    return R


def start(N: int, S: int, query=0) -> torch.Tensor:
    """One-hot of token `query`, or the uniform vector for query None -> [S, N]."""
    r0 = torch.zeros((S, N), dtype=torch.float64)
    if query is None:
        r0 += 1.0 / N
    else:
        r0[:, query] = 1.0
    return r0


def rollout(layers, rho: float = 0.5, r0: torch.Tensor = None, query=0) -> torch.Tensor:
    """r = r0^T R [S, N]; r0 defaults to the one-hot of `query` (None: uniform)."""
    R = rollout_matrix(layers, rho)
    if r0 is None:
        r0 = start(R.shape[-1], R.shape[0], query)
    return torch.einsum("si,sij->sj", r0.double(), R)


def step(q, k, scale: float, r_in: torch.Tensor, rho: float = 0.5) -> torch.Tensor:
    """One layer applied to a row, through the full matrix: r_in^T Ahat."""
    return torch.einsum("si,sij->sj", r_in.double(), layer_matrix(q, k, scale, rho))


def video(r_space: torch.Tensor, r_time: torch.Tensor):
    """r_space [B*T, n + 1], r_time [B, T + 1] -> (space [B, T, n], time [B, T], video [B, T, n], scaled [B, T, n])."""
    B, T = r_time.shape[0], r_time.shape[1] - 1
    space = r_space.double().view(B, T, -1)[:, :, 1:]
    time = r_time.double()[:, 1:]
    vid = time[:, :, None] * space
    scaled = cam_ref.scale(vid.reshape(B, -1)).view(vid.shape)
    return space, time, vid, scaled


# ---------------------------------------------------------------- Q and K of the models
def split_heads(qkv: torch.Tensor, heads: int):
    """to_qkv output [S, N, 3 h dh] -> q, k [S, H, N, dh] (chunks of the last dim, heads the outer factor of each chunk)."""
    S, N, three = qkv.shape
    dh = three // 3 // heads
    q, k, _ = qkv.view(S, N, 3, heads, dh).permute(2, 0, 3, 1, 4)
    return q, k


def vivit_layers(space_qkv, time_qkv, heads: int):
    """Hooked to_qkv outputs of the two stacks -> ([(q, k, scale)] space, the same for time)."""
    def stack(outs):
        ls = []
        for o in outs:
            q, k = split_heads(o, heads)
            ls.append((q, k, q.shape[-1] ** -0.5))
        return ls
    return stack(space_qkv), stack(time_qkv)


def vivit_rollout(space_qkv, time_qkv, heads: int, rho: float = 0.5, pool: str = "cls"):
    """-> (r_space [b t, n + 1], r_time [b, t + 1], video [b, t, n]) float64."""
    sp, tm = vivit_layers(space_qkv, time_qkv, heads)
    r_space = rollout(sp, rho)
    r_time = rollout(tm, rho, query=None if pool == "mean" else 0)
    return r_space, r_time, video(r_space, r_time)[2]


def fixture_conditions(r_space, space_qkv, time_qkv, heads: int, rho: float):
    """What makes a rollout fixture able to tell a wrong kernel from a right one -> (the minimum over the frames of the patch
    max / min of r_space, the minimum over the two stacks and their sequences of |right - rollout with every layer's keys
    rotated by one| relative to the right one's maximum, max |scale q . k| over all layers)."""
    patches = r_space[:, 1:]
    ratio = float((patches.max(1).values / patches.min(1).values).min())
    sp, tm = vivit_layers(space_qkv, time_qkv, heads)
    rot = lambda ls: [(q, torch.roll(k, 1, dims=2), s) for q, k, s in ls]
    diffs = []
    for ls in (sp, tm):
        good, bad = rollout(ls, rho), rollout(rot(ls), rho)
        diffs.append(float(((good - bad).abs().amax(1) / good.amax(1)).min()))
    smax = max(float((torch.einsum("shid,shjd->shij", q.double(), k.double()) * s).abs().max()) for q, k, s in sp + tm)
    return ratio, min(diffs), smax


def hook_to_qkv(model):
    """Forward hooks on every ``to_qkv`` of a reference-layout ViViT -> (space outputs, time outputs, handles)."""
    space, time, handles = [], [], []
    for name, m in model.named_modules():
        if name.endswith("to_qkv"):
            dst = space if name.startswith("space_transformer") else time
            handles.append(m.register_forward_hook(lambda _m, _i, o, dst=dst: dst.append(o.detach())))
    return space, time, handles


def torch_encoder_layers(encoder: torch.nn.TransformerEncoder, x: torch.Tensor):
    """Q and K of every layer of torch's own nn.TransformerEncoder (post-norm, seq-first x [L, B, E]): forward pre-hooks
    record each layer's input, the layer's in_proj weights give q and k -> [(q, k, scale)] with q, k [B, H, L, dh]."""
    inputs, handles = [], []
    for layer in encoder.layers:
        handles.append(layer.register_forward_pre_hook(lambda _m, args, inputs=inputs: inputs.append(args[0].detach())))
    with torch.no_grad():
        encoder(x)
    for h in handles:
        h.remove()
    out = []
    for layer, xin in zip(encoder.layers, inputs):
        a = layer.self_attn
        E, H = a.embed_dim, a.num_heads
        dh = E // H
        proj = xin.double() @ a.in_proj_weight.detach().double().t() + a.in_proj_bias.detach().double()      # [L, B, 3E]
        Lq, B = xin.shape[0], xin.shape[1]
        q = proj[..., :E].view(Lq, B, H, dh).permute(1, 2, 0, 3)
        k = proj[..., E:2 * E].view(Lq, B, H, dh).permute(1, 2, 0, 3)
        out.append((q, k, dh ** -0.5))
    return out


def rel_l2(a, b) -> float:
    a = torch.as_tensor(np.asarray(a), dtype=torch.float64) if not isinstance(a, torch.Tensor) else a.detach().double().cpu()
    b = torch.as_tensor(np.asarray(b), dtype=torch.float64) if not isinstance(b, torch.Tensor) else b.detach().double().cpu()
    return float((a - b).norm() / b.norm())
