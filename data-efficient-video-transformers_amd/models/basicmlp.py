"""Mirror of the reference's ``src/models/basicmlp.py``: ``BasicMLP``, the supervised MLP baseline on expert embeddings:
fc1 -> ReLU -> fc2 -> ReLU -> BatchNorm1d(1024) -> fc3 -> ReLU (the embedding) -> fc4 (305 classes), trained with
``nn.CrossEntropyLoss()`` and ``Adam`` without weight decay.

Kept: the constructor (one ``config``: confuse-style ``config["k"].get()`` as the reference reads it, or a plain dict),
the attributes (``fc1`` .. ``fc4``, ``batchnorm``, ``softmax``, ``loss``, ``config`` ...), the state-dict keys and the
initialisation draw order.  ``BatchNorm1d(1024)`` is hard-coded as in the reference: a ``bottle_neck`` other than 1024
fails in ``forward`` with torch's message.  The loss is the mean over the labels that are not ``-100``
(``ignore_index``); ``nn.LogSoftmax`` is built and unused, as in the reference.

All arithmetic is HIP (``functional.mlp_chain``: GEMMs with bias / ReLU epilogues, ``dvt_bn1d_relu_*``; the loss on
``dvt_ce_labels_*``; ``nn.CrossEntropyLoss(label_smoothing=s)`` with s > 0, and float ``[M, C]`` labels, on ``dvt_targets_mix``
+ ``dvt_ce_soft_*``, where every row counts: there ``ignore_index`` is not honoured -- a non-default one is refused, a label of -100 makes the
loss NaN).
``compute_dtype`` (attribute, default bf16) sets the activation dtype; fp32 is exact fp32 arithmetic.

Deliberate deviations: the torchmetrics ``f1`` / ``acc`` objects, unused by the reference's steps, are
not constructed here (``metrics.F1`` is the device-side stand-in: ``model.f1 = metrics.F1(22)``); ``validation_step`` does not print the outputs and labels.
"""
from __future__ import annotations

import torch
from torch import nn

from .. import functional as F
from .. import ops
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
                and 0.0 <= L.label_smoothing < 1.0):
            raise NotImplementedError(f"BasicMLP: only nn.CrossEntropyLoss(label_smoothing=s) (mean, no weight) has a HIP "
                                      f"kernel, got {L!r}")
        soft = labels.is_floating_point()
        if not soft and L.label_smoothing == 0.0:
            return F.cross_entropy(output, labels, L.ignore_index)
        if soft and L.label_smoothing != 0.0:
            raise NotImplementedError("BasicMLP: label_smoothing on class-probability labels is not built; smooth the integer "
                                      "labels (input_stage.Mixup does) or pass label_smoothing=0")
        # smoothed one-hot rows (or the caller's mixed rows, as they are) through the soft-target loss: every row counts, so
        # a label outside [0, C) -- ignore_index among them -- makes the loss NaN instead of being skipped.  Asking for an
        # ignore_index of one's own states that such labels are there: that is refused (the default cannot be told from
        # "none" without reading the labels back from the device)
        if L.ignore_index != ops.CE_IGNORE_INDEX:
            raise NotImplementedError(f"BasicMLP: ignore_index={L.ignore_index} is honoured on integer labels without label "
                                      "smoothing only; the soft-target loss counts every row")
        M = labels.shape[0]
        ident = torch.zeros(M, 8, dtype=torch.int32)
        ident[:, 0] = torch.arange(M, dtype=torch.int32)
        targets = ops.targets_mix(ident, torch.ones(M), y=labels.float() if soft else None, labels=None if soft else labels,
                                  num_classes=output.shape[1], smoothing=L.label_smoothing)
        return F.soft_target_cross_entropy(output, targets)

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
