"""Mirror of the reference's ``src/models/basicmlp.py``: ``BasicMLP``, the supervised MLP baseline on expert embeddings:
fc1 -> ReLU -> fc2 -> ReLU -> BatchNorm1d(1024) -> fc3 -> ReLU (the embedding) -> fc4 (305 classes), trained with
``nn.CrossEntropyLoss()`` and ``Adam`` without weight decay.

Kept: the constructor (one ``config``: confuse-style ``config["k"].get()`` as the reference reads it, or a plain dict),
the attributes (``fc1`` .. ``fc4``, ``batchnorm``, ``softmax``, ``loss``, ``config`` ...), the state-dict keys and the
initialisation draw order.  ``BatchNorm1d(1024)`` is hard-coded as in the reference: a ``bottle_neck`` other than 1024
fails in ``forward`` with torch's message.  The loss is the mean over the labels that are not ``-100``
(``ignore_index``); ``nn.LogSoftmax`` is built and unused, as in the reference.

All arithmetic is HIP (``functional.mlp_chain``: GEMMs with bias / ReLU epilogues, ``dvt_bn1d_relu_*``; the loss on
``dvt_ce_labels_*``).  ``compute_dtype`` (attribute, default bf16) sets the activation dtype; fp32 is exact fp32 arithmetic.

Deliberate deviations: the torchmetrics ``f1`` / ``acc`` objects, unused by the reference's steps, are
not constructed here (``metrics.F1`` is the device-side stand-in: ``model.f1 = metrics.F1(22)``); ``validation_step`` does not print the outputs and labels.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import functional as F
from .. import optim
from ..lightning_compat import LightningModule
from .contrastivemodel import cfg, rows_input


class BasicMLP(LightningModule):
    def __init__(self, config):
        super(BasicMLP, self).__init__()
        self.input_layer_size = cfg(config, "input_shape")
        self.bottleneck_size = cfg(config, "bottle_neck")
        self.output_layer_size = cfg(config, "output_shape")
        self.batch_size = cfg(config, "batch_size")
        self.config = config
        self.softmax = nn.LogSoftmax(dim=-1)
        self.compute_dtype = torch.bfloat16

        self.fc1 = nn.Linear(self.input_layer_size, self.input_layer_size)
        self.batchnorm = nn.BatchNorm1d(1024)
        self.fc2 = nn.Linear(self.input_layer_size, self.bottleneck_size)
        self.fc3 = nn.Linear(self.bottleneck_size, self.bottleneck_size)
        self.fc4 = nn.Linear(self.bottleneck_size, 305)
        self.loss = nn.CrossEntropyLoss()

    def _layers(self):
        return [F.MlpLayer("linear", self.fc1, relu=True), F.MlpLayer("linear", self.fc2),
                F.MlpLayer("bn_relu", self.batchnorm), F.MlpLayer("linear", self.fc3, relu=True),
                F.MlpLayer("linear", self.fc4, out_f32=True)]

    def forward(self, tensor):
        """Logits [B, 305] (fp32)."""
        if self.bottleneck_size != self.batchnorm.num_features:      # what nn.BatchNorm1d(1024) raises in the reference
            raise RuntimeError(f"running_mean should contain {self.bottleneck_size} elements not "
                               f"{self.batchnorm.num_features}")
        x = F.cast(tensor, self.compute_dtype)
        (out,) = F.mlp_chain(x, self._layers(), segments=1, training=self.training)
        return out

    def configure_optimizers(self):
        return optim.Adam(self.parameters(), lr=cfg(self.config, "learning_rate"))

    def expert_aggregation(self, expert_list):
        agg = cfg(self.config, "aggregation")
        if agg in ("avg_pool", "mean_pool"):
            raise NotImplementedError(f"expert_aggregation({agg!r}) is broken in the reference and is not built")
        if agg == "concat":
            lead = tuple(expert_list[0].shape[:-1])
            n, D = int(torch.Size(lead).numel()), sum(t.shape[-1] for t in expert_list)
            rows = [[t.reshape(n, -1)[r] for t in expert_list] for r in range(n)]
            return rows_input(rows, D, expert_list[0].dtype, expert_list[0].device).view(*lead, D)
        return expert_list

    def debug(self, x_i, x_j):
        for keys, values in x_i.items():
            print(keys, values.shape)

    def criterion(self, output, labels):
        L = self.loss
        if not (isinstance(L, nn.CrossEntropyLoss) and L.reduction == "mean" and L.weight is None
                and L.label_smoothing == 0.0):
            raise NotImplementedError(f"BasicMLP: only nn.CrossEntropyLoss() (mean, no weight, no smoothing) has a HIP "
                                      f"kernel, got {L!r}")
        return F.cross_entropy(output, labels, L.ignore_index)

    def _batch(self, batch):
        dev = next(self.parameters()).device
        x = rows_input([[t.reshape(-1)] for t in batch["x_i_experts"]], self.input_layer_size, self.compute_dtype, dev)
        labels = batch["label"]
        labels = (labels if isinstance(labels, torch.Tensor) else torch.tensor(labels)).to(dev, torch.int64).reshape(-1)
        return x, labels

    def training_step(self, batch, batch_idx):
        x, labels = self._batch(batch)
        loss = self.criterion(self(x), labels)
        self.log("training loss", loss, on_step=True, on_epoch=True)
        return loss

    def validation_step(self, batch, batch_idx):
        x, labels = self._batch(batch)
        loss = self.criterion(self(x), labels)
        self.log("validation loss", loss, on_step=True, on_epoch=True)
        return loss
