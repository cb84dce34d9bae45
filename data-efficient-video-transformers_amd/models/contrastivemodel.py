"""Mirror of the reference's ``src/models/contrastivemodel.py``: ``SpatioTemporalContrastiveModel``, the self-supervised
MLP that trains on the expert embeddings of ``models.pretrained.EmbeddingExtractor`` with the NT-Xent ``ContrastiveLoss``.

Kept: the constructor (one ``config`` mapping: plain dict or confuse-style views), the attributes (``encoder_net``,
``projector_net``, ``loss``, ``config``, ``train_iters_per_epoch``, ``running_logits``, ``running_labels``, ``proj_list``,
``label_list`` ...), the module trees -- so parameter names, state-dict keys (``encoder_net.2.running_mean`` ...) and the
initialisation draw order are the reference's -- and its semantics:
  - BatchNorm1d reads the RECTIFIED first Linear (Linear -> ReLU -> BatchNorm1d, :28-30);
  - ``forward`` returns the rectified embedding: the projector's first ``ReLU(inplace=True)`` overwrites the encoder's
    output tensor, so what the reference returns (:49-55, stored by ``test_step``) is relu(Linear_3(...));
  - two forward passes per step, each view with its own BatchNorm statistics; the running statistics move twice (view i,
    then view j) and ``num_batches_tracked`` grows by 2 (:160-161);
  - ``training_step`` L2-normalises both outputs before the loss, ``validation_step`` does not (:160-166, :190-196);
  - ``configure_optimizers``: Adam(lr, weight_decay) with coupled decay and ``LinearWarmupCosineAnnealingLR(
    warmup_epochs=epochs // 10, max_epochs=epochs)`` (:57-92); the additive config key ``optimizer: "lars"`` selects the
    reference's commented-out LARS block instead, with the same scheduler.

All arithmetic is HIP: the GEMMs (bias and ReLU in their epilogues), ``dvt_bn1d_relu_*``, dropout, L2-normalisation and the
contrastive loss.  ``step_views(x_i, x_j)`` runs both views as ONE [2B, .] launch per layer and returns what two
``forward`` calls return; ``training_step`` uses it.  ``compute_dtype`` (attribute, default bf16) sets the activation dtype;
fp32 is exact fp32 arithmetic.

Deliberate deviations:
  - ``expert_aggregation``: ``"mean_pool"`` (a NameError in the reference), ``"avg_pool"`` (ill-formed) and
    ``"collab_gate"`` (returns the list unchanged, which the following ``torch.stack`` cannot take) raise
    ``NotImplementedError``.
  - Training-mode dropout draws its masks from the Philox kernel: torch's generator stream is not reproduced.
"""
from __future__ import annotations

import math

import torch
from torch import nn

from .. import functional as F
from .. import ops
from .. import optim
from ..lightning_compat import LightningModule
from ..lr_scheduler import LinearWarmupCosineAnnealingLR
from .losses.ntxent import ContrastiveLoss

AGGREGATIONS = ("none", "concat")
_UNBUILT = {
    "avg_pool": "expert_aggregation('avg_pool') is ill-formed in the reference (adaptive_avg_pool2d of a row to "
                "input_shape) and is not built",
    "mean_pool": "expert_aggregation('mean_pool') raises NameError in the reference (`size` is undefined) and is not built",
    "collab_gate": "expert_aggregation('collab_gate') returns the expert list unchanged in the reference, which the step "
                   "cannot stack; it is not built",
}


def cfg(config, key):
    """config[key] of a plain mapping or of a confuse-style configuration (whose views resolve through ``.get()``)."""
    v = config[key]
    if not isinstance(v, (dict, str, bytes)) and callable(getattr(v, "get", None)):
        return v.get()
    return v


def rows_input(rows, D: int, dtype: torch.dtype, device) -> torch.Tensor:
    """[len(rows), D] in ``dtype`` on ``device`` from per-row lists of expert tensors: GPU tensors in ONE gather launch
    (``dvt_gather_rows_ptr``), host tensors concatenated on the host and copied once."""
    if all(t.is_cuda for r in rows for t in r):
        return ops.gather_rows_ptr([[t.contiguous() for t in r] for r in rows], D, dtype, device)
    host = torch.cat([t.detach().reshape(-1).float().cpu() for r in rows for t in r])
    if host.numel() != len(rows) * D:
        raise ValueError(f"expert rows hold {host.numel()} elements, expected {len(rows)} x {D}")
    x = host.view(len(rows), D).to(device)
    return x if dtype == torch.float32 else ops.cast(x, dtype)


class SpatioTemporalContrastiveModel(LightningModule):
    def __init__(self, config):
        super().__init__()
        self.input_layer_size = cfg(config, "input_shape")
        self.hidden_layer_size = cfg(config, "hidden_layer")
        self.projection_size = cfg(config, "projection_size")
        self.output_layer_size = cfg(config, "output_shape")
        self.batch_size = cfg(config, "batch_size")
        self.num_samples = cfg(config, "num_samples")
        self.config = config
        self.train_iters_per_epoch = self.num_samples // self.batch_size
        self.running_logits = []
        self.running_labels = []
        self.compute_dtype = torch.bfloat16

        self.encoder_net = nn.Sequential(
            nn.Linear(self.input_layer_size, self.hidden_layer_size, bias=False),
            nn.ReLU(inplace=True),
            nn.BatchNorm1d(self.hidden_layer_size),
            nn.Linear(self.hidden_layer_size, self.hidden_layer_size, bias=False),
            nn.ReLU(inplace=True),
            nn.Linear(self.hidden_layer_size, self.projection_size),
        )
        self.projector_net = nn.Sequential(
            nn.ReLU(inplace=True),
            nn.Linear(self.projection_size, self.projection_size),
            nn.ReLU(inplace=True),
            nn.Dropout(p=0.1),
            nn.Linear(self.projection_size, self.output_layer_size),
        )
        self.loss = ContrastiveLoss(self.batch_size)
        self.proj_list = []
        self.label_list = []

    # ------------------------------------------------------------------ network
    def _layers(self):
        e, p = self.encoder_net, self.projector_net
        return [F.MlpLayer("linear", e[0]), F.MlpLayer("bn_relu", e[2]), F.MlpLayer("linear", e[3], relu=True),
                F.MlpLayer("linear", e[5], relu=True),              # + the projector's ReLU(inplace): the embedding
                F.MlpLayer("linear", p[1], relu=True), F.MlpLayer("dropout", p=p[3].p),
                F.MlpLayer("linear", p[4], out_f32=True)]

    def _run(self, x, segments):
        x = F.cast(x, self.compute_dtype)
        return F.mlp_chain(x, self._layers(), segments=segments, training=self.training, returned=(3, 6))

    def forward(self, tensor):
        """-> (embedding [B, projection_size] in compute dtype, rectified; output [B, output_shape] fp32)."""
        return self._run(tensor, 1)

    def step_views(self, x_i, x_j):
        """Both views through every layer as one [2B, .] launch (BatchNorm with per-view statistics) ->
        ((embedding_i, output_i), (embedding_j, output_j)), what ``self(x_i)`` then ``self(x_j)`` return."""
        B = x_i.shape[0]
        if x_j.shape != x_i.shape:
            raise ValueError("step_views: the two views need equal shapes")
        emb, out = self._run(F.concat_rows(F.cast(x_i, self.compute_dtype), F.cast(x_j, self.compute_dtype)), 2)
        return (emb[:B], out[:B]), (emb[B:], out[B:])

    # ------------------------------------------------------------------ optimisation
    def configure_optimizers(self):
        """Adam, as the reference runs; config key ``optimizer: "lars"`` (ours, optional) selects the block the reference
        keeps commented out (:64-70): LARS over ``exclude_from_wt_decay``'s two groups with ``config["momentum"]``."""
        which = cfg(self.config, "optimizer") if "optimizer" in self.config else "adam"
        if which == "adam":
            optimizer = optim.Adam(self.parameters(), lr=cfg(self.config, "learning_rate"),
                                   weight_decay=cfg(self.config, "weight_decay"))
        elif which == "lars":
            parameters = self.exclude_from_wt_decay(self.named_parameters(), weight_decay=cfg(self.config, "weight_decay"))
            optimizer = optim.LARS(parameters, lr=cfg(self.config, "learning_rate"), momentum=cfg(self.config, "momentum"),
                                   weight_decay=cfg(self.config, "weight_decay"), trust_coefficient=0.0001)
        else:
            raise ValueError(f"config optimizer: {which!r} is not one of 'adam', 'lars'")
        epochs = cfg(self.config, "epochs")
        scheduler = LinearWarmupCosineAnnealingLR(optimizer, warmup_epochs=epochs // 10, max_epochs=epochs)
        return [optimizer], [scheduler]

    def exclude_from_wt_decay(self, named_params, weight_decay, skip_list=['bias', 'bn']):
        params, excluded_params = [], []
        for name, param in named_params:
            if not param.requires_grad:
                continue
            if any(layer_name in name for layer_name in skip_list):
                excluded_params.append(param)
            else:
                params.append(param)
        return [{'params': params, 'weight_decay': weight_decay}, {'params': excluded_params, 'weight_decay': 0.}]

    # ------------------------------------------------------------------ batches
    def _aggregation(self):
        agg = cfg(self.config, "aggregation")
        if agg in _UNBUILT:
            raise NotImplementedError(_UNBUILT[agg])
        if agg not in AGGREGATIONS:
            raise NotImplementedError(f"expert_aggregation: unknown mode {agg!r} (built: {', '.join(AGGREGATIONS)})")
        return agg

    def expert_aggregation(self, expert_list):
        """One sample's experts -> its input row: ``"none"`` the first expert, ``"concat"`` all of them along the last
        dimension."""
        agg = self._aggregation()
        if agg == "none":
            return expert_list[0]
        lead = tuple(expert_list[0].shape[:-1])
        if any(tuple(t.shape[:-1]) != lead for t in expert_list):
            raise ValueError("expert_aggregation('concat'): experts differ in their leading dimensions")
        n, D = math.prod(lead), sum(t.shape[-1] for t in expert_list)
        dtype = expert_list[0].dtype if expert_list[0].dtype in (torch.float32, torch.bfloat16, torch.float16) else torch.float32
        rows = [[t.reshape(n, -1)[r] for t in expert_list] for r in range(n)]
        return rows_input(rows, D, dtype, expert_list[0].device).view(*lead, D)

    def _views(self, views):
        """[S*B, input_shape] in compute dtype from S lists of per-sample expert lists (the contrastive collate:
        MMX_Contrastive_dl.py:29-32), all views in one gather."""
        agg = self._aggregation()
        rows = [[t.reshape(-1) for t in (experts[:1] if agg == "none" else experts)] for view in views for experts in view]
        dev = next(self.parameters()).device
        return rows_input(rows, self.input_layer_size, self.compute_dtype, dev)

    def debug(self, x_i, x_j):
        for keys, values in x_i.items():
            print(keys, values.shape)

    def _loss_rows(self, out):
        if not isinstance(self.loss, ContrastiveLoss):
            raise NotImplementedError(f"SpatioTemporalContrastiveModel: only ContrastiveLoss has a HIP kernel, got "
                                      f"{type(self.loss).__name__}")
        if out.shape[0] != 2 * self.loss.batch_size:
            raise ValueError(f"expected two views of {self.loss.batch_size} rows, got {out.shape[0]} rows")
        return F.contrastive_loss_rows(out, self.loss._t)

    def training_step(self, batch, batch_idx):
        x = self._views((batch["x_i_experts"], batch["x_j_experts"]))
        _, out = self._run(x, 2)
        loss = self._loss_rows(F.l2_normalize(out))
        self.log("train/contrastive/loss", loss)
        return loss

    def validation_step(self, batch, batch_idx):
        x = self._views((batch["x_i_experts"], batch["x_j_experts"]))
        emb, out = self._run(x, 2)
        loss = self._loss_rows(out)
        self.log("val/contrastive/loss", loss)
        return {"loss": loss, "val_outputs": emb[:x.shape[0] // 2]}

    def test_step(self, batch, batch_idx):
        x = self._views((batch["x_i_experts"],))
        label = batch["label"]
        x_i_embeddings, _ = self(x)
        self.proj_list.append(x_i_embeddings.squeeze())
        self.label_list.append(label)
        return {"length": len(self.proj_list)}
