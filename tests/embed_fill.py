"""Parameter and running-statistic fills for the expert-embedding tests, shared with tools/gen_golden_embed.py."""
import numpy as np
import torch

from tests.util import fill_resnet_from_numpy

RESNET50_SEED = 2048          # tests/golden/embed_resnet50.npz: weights from this seed (stored nowhere)


def fill_running_stats(net, rng) -> None:
    """Non-trivial eval BatchNorm statistics: running_mean 0.1 n, running_var 0.5 + u[0, 1), in ``named_buffers()`` order."""
    with torch.no_grad():
        for name, b in net.named_buffers():
            if name.endswith("running_mean"):
                b.copy_(torch.from_numpy(np.float32(0.1) * rng.standard_normal(tuple(b.shape)).astype(np.float32)))
            elif name.endswith("running_var"):
                b.copy_(torch.from_numpy(np.float32(0.5) + rng.random(tuple(b.shape)).astype(np.float32)))


def fill_resnet50(net, seed: int = RESNET50_SEED) -> None:
    rng = np.random.default_rng(seed)
    fill_resnet_from_numpy(net, rng)
    fill_running_stats(net, rng)


def fill_video_net(net, seed: int) -> None:
    """He-scaled 5-D convolution weights (fan-out), 1 + 0.1 n BN scales, 0.1 n shifts, 0.02 n for fc; then the running
    statistics.  ``named_parameters()`` order from one numpy Generator (tests/util.fill_resnet_from_numpy is 4-D only)."""
    rng = np.random.default_rng(seed)
    with torch.no_grad():
        for name, p in net.named_parameters():
            a = rng.standard_normal(tuple(p.shape)).astype(np.float32)
            if p.dim() == 5:
                a *= np.float32(np.sqrt(2.0 / (p.shape[0] * p.shape[2] * p.shape[3] * p.shape[4])))
            elif p.dim() == 2:
                a *= np.float32(0.02)
            elif name.endswith("weight"):
                a = 1 + np.float32(0.1) * a
            else:
                a = np.float32(0.1) * a
            p.copy_(torch.from_numpy(a))
    fill_running_stats(net, rng)


def resnet50_input(seed: int = RESNET50_SEED + 1, n: int = 2, size: int = 224) -> torch.Tensor:
    return torch.from_numpy(np.random.default_rng(seed).standard_normal((n, 3, size, size)).astype(np.float32))
