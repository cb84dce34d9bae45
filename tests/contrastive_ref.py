"""Torch-CPU restatement of the two embedding MLPs (src/models/contrastivemodel.py, src/models/basicmlp.py) written from
their documented semantics, in float64: what the fixture tests/golden/contrastive_mlp.npz means, and the yardstick of
the GPU tests."""
from __future__ import annotations

import torch
import torch.nn.functional as TF


def bn_relu(z, g, b, rm, rv, training, eps=1e-5, momentum=0.1):
    """BatchNorm1d(relu(z)); rm / rv updated in place (training) as nn.BatchNorm1d does."""
    a = torch.relu(z)
    if training:
        mean, var = a.mean(0), a.var(0, unbiased=False)
        with torch.no_grad():
            n = a.shape[0]
            rm.mul_(1 - momentum).add_(momentum * mean.detach().to(rm.dtype))
            rv.mul_(1 - momentum).add_(momentum * (var.detach() * n / (n - 1)).to(rv.dtype))
    else:
        mean, var = rm.to(a.dtype), rv.to(a.dtype)
    return (a - mean) / torch.sqrt(var + eps) * g + b


def contrastive_forward(P, x, stats, training=True):
    """-> (embedding, output) of SpatioTemporalContrastiveModel (dropout p = 0); stats = [running_mean, running_var]."""
    z = x @ P["encoder_net.0.weight"].T
    y = bn_relu(z, P["encoder_net.2.weight"], P["encoder_net.2.bias"], stats[0], stats[1], training)
    h = torch.relu(y @ P["encoder_net.3.weight"].T)
    e = torch.relu(h @ P["encoder_net.5.weight"].T + P["encoder_net.5.bias"])
    p = torch.relu(e @ P["projector_net.1.weight"].T + P["projector_net.1.bias"])
    return e, p @ P["projector_net.4.weight"].T + P["projector_net.4.bias"]


def ntxent(zi, zj, temperature=0.5):
    """ContrastiveLoss(batch_size).forward (ntxent.py:53-75)."""
    B = zi.shape[0]
    reps = torch.cat([zi, zj], 0)
    sim = TF.cosine_similarity(reps.unsqueeze(1), reps.unsqueeze(0), dim=2)
    pos = torch.cat([torch.diag(sim, B), torch.diag(sim, -B)])
    mask = (~torch.eye(2 * B, dtype=torch.bool)).to(sim.dtype)
    den = (mask * torch.exp(sim / temperature)).sum(1)
    return torch.sum(-torch.log(torch.exp(pos / temperature) / den)) / (2 * B)


def contrastive_step(P, x_i, x_j, stats, normalize=True):
    """training_step: two forward passes (view i first), L2-normalised outputs, the loss."""
    _, oi = contrastive_forward(P, x_i, stats)
    _, oj = contrastive_forward(P, x_j, stats)
    if normalize:
        oi, oj = TF.normalize(oi), TF.normalize(oj)
    return ntxent(oi, oj)


def mlp_forward(P, x, stats, training=True):
    h = torch.relu(x @ P["fc1.weight"].T + P["fc1.bias"])
    z = h @ P["fc2.weight"].T + P["fc2.bias"]
    y = bn_relu(z, P["batchnorm.weight"], P["batchnorm.bias"], stats[0], stats[1], training)
    e = torch.relu(y @ P["fc3.weight"].T + P["fc3.bias"])
    return e @ P["fc4.weight"].T + P["fc4.bias"]


def params64(module):
    """float64 leaf copies of a module's parameters (requires_grad) keyed by name."""
    return {k: v.detach().cpu().double().requires_grad_(True) for k, v in module.named_parameters()}
