"""``LinearWarmupCosineAnnealingLR`` of pl_bolts (``pl_bolts.optimizers.lr_scheduler``), which the reference's
SpatioTemporalContrastiveModel.configure_optimizers builds (contrastivemodel.py:83) with ``warmup_epochs = epochs // 10``
and ``max_epochs = epochs``, stepped once per epoch.

pl_bolts is not a dependency; the rule below is pl_bolts' chained ``get_lr`` as stated in DESIGN.md §4.12 (written from
the package's published behaviour, not checked against its source).  With warmup w, maximum M, start s, floor eta:

    epoch 0            -> s
    0 < e < w          -> lr + (base - s) / (w - 1)
    e == w             -> base
    (e - 1 - M) % (2 (M - w)) == 0 -> lr + (base - eta) (1 - cos(pi / (M - w))) / 2     (periodic restart)
    otherwise          -> (1 + cos(pi (e - w) / (M - w))) / (1 + cos(pi (e - w - 1) / (M - w))) (lr - eta) + eta

and the closed form (``step(epoch)``, ``_get_closed_form_lr``):

    e < w  -> s + e (base - s) / max(1, w - 1)
    else   -> eta + (base - eta) (1 + cos(pi (e - w) / (M - w))) / 2

They agree at every epoch when w >= 1.  With w = 0 (``epochs < 10`` in the reference) the chained rule stays at s (0 by
default) at every epoch up to M -- the cosine ratio multiplies lr - eta = 0 -- and only the periodic-restart branch at
M + 1 moves it; the closed form does not stay there.  The chained form is what ``step()`` follows.

Every ``step()`` also writes the new rates into the device LR scalars of the HIP optimizers (``optim.Adam``), so a
training step captured in a hipGraph picks up each epoch's rate without re-capture.
"""
from __future__ import annotations

import math

from torch.optim.lr_scheduler import LRScheduler


class LinearWarmupCosineAnnealingLR(LRScheduler):
    def __init__(self, optimizer, warmup_epochs: int, max_epochs: int, warmup_start_lr: float = 0.0,
                 eta_min: float = 0.0, last_epoch: int = -1):
        self.warmup_epochs = int(warmup_epochs)
        self.max_epochs = int(max_epochs)
        self.warmup_start_lr = float(warmup_start_lr)
        self.eta_min = float(eta_min)
        super().__init__(optimizer, last_epoch)

    def get_lr(self):
        e, w, M = self.last_epoch, self.warmup_epochs, self.max_epochs
        s, eta = self.warmup_start_lr, self.eta_min
        groups = self.optimizer.param_groups
        if e == 0:
            return [s] * len(self.base_lrs)
        if e < w:
            return [g["lr"] + (base - s) / (w - 1) for base, g in zip(self.base_lrs, groups)]
        if e == w:
            return list(self.base_lrs)
        if (e - 1 - M) % (2 * (M - w)) == 0:
            return [g["lr"] + (base - eta) * (1 - math.cos(math.pi / (M - w))) / 2
                    for base, g in zip(self.base_lrs, groups)]
        return [(1 + math.cos(math.pi * (e - w) / (M - w))) / (1 + math.cos(math.pi * (e - w - 1) / (M - w)))
                * (g["lr"] - eta) + eta for g in groups]

    def _get_closed_form_lr(self):
        e, w, M = self.last_epoch, self.warmup_epochs, self.max_epochs
        s, eta = self.warmup_start_lr, self.eta_min
        if e < w:
            return [s + e * (base - s) / max(1, w - 1) for base in self.base_lrs]
        return [eta + 0.5 * (base - eta) * (1 + math.cos(math.pi * (e - w) / (M - w))) for base in self.base_lrs]

    def step(self, epoch=None):
        super().step(epoch)
        sync = getattr(self.optimizer, "sync_lr", None)
        if sync is not None:
            sync()
