#!/usr/bin/env python3
"""Generate tests/golden/contrastive_mlp.npz from the *imported reference* (build container only):

    python tools/gen_golden_contrastive.py

Executes the reference's ``src/models/contrastivemodel.py`` and ``src/models/basicmlp.py`` (loaded by file path, never
copied) with generator-only stand-ins registered in ``sys.modules`` for the duration of the script:
``pytorch_lightning`` (LightningModule = nn.Module with a no-op ``log`` and a ``device``), ``pl_bolts`` (the scheduler and
LARS names the module imports; neither is called here), ``torchmetrics`` (F1 / Accuracy names) and a confuse-style
configuration (``config["k"].get()``) for BasicMLP.  ``models.losses.ntxent`` is the reference's own file.

Stored (data only), at small odd shapes with the projector's dropout set to p = 0:
  * SpatioTemporalContrastiveModel: the fill seed (weights: ``tests.util.fill_state_from_numpy``), the two views' expert
    rows, ``forward(x_i)`` -> (embedding, output) on a copy in training mode, the training_step loss, every parameter
    gradient and the BatchNorm running statistics after the step;
  * BasicMLP (bottle_neck 1024, as its hard-coded BatchNorm1d(1024) requires): seed, inputs, labels with -100 entries,
    the logits, the training_step loss, the gradients (fc3 / fc4 weights: norm and first 32 rows) and the running statistics.
"""
from __future__ import annotations

import copy
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests.util import fill_state_from_numpy  # noqa: E402

REF = "/root/reference/src/models"
OUT = os.path.join(ROOT, "tests", "golden", "contrastive_mlp.npz")

SEED = 1130
# contrastive shapes: 3 experts of odd widths concatenated (D = 40), B = 6 per view
CT = dict(input_shape=40, hidden_layer=70, projection_size=37, output_shape=19, batch_size=6, num_samples=60,
          aggregation="concat", learning_rate=1e-3, weight_decay=0.09, epochs=500)
EXPERTS = (24, 11, 5)
MLP = dict(input_shape=40, bottle_neck=1024, output_shape=305, batch_size=7, learning_rate=5e-6, aggregation="concat")
MLP_LABELS = [3, -100, 304, 0, 17, -100, 150]


def _load(name, path):
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _View:                       # confuse-style view: config["k"].get()
    def __init__(self, v):
        self.v = v

    def get(self):
        return self.v


def _stand_ins():
    pl = types.ModuleType("pytorch_lightning")

    class LightningModule(torch.nn.Module):
        def log(self, *a, **k):
            pass

        @property
        def device(self):
            return next(self.parameters()).device

    pl.LightningModule = LightningModule
    bolts = types.ModuleType("pl_bolts")
    bopt = types.ModuleType("pl_bolts.optimizers")
    bsched = types.ModuleType("pl_bolts.optimizers.lr_scheduler")
    blars = types.ModuleType("pl_bolts.optimizers.lars")
    bsched.LinearWarmupCosineAnnealingLR = object
    blars.LARS = object
    tm = types.ModuleType("torchmetrics")
    tm.F1 = lambda **k: None
    tm.Accuracy = lambda **k: None
    models = types.ModuleType("models")
    losses = types.ModuleType("models.losses")
    ntx = _load("models.losses.ntxent", os.path.join(REF, "losses", "ntxent.py"))
    return {"pytorch_lightning": pl, "pl_bolts": bolts, "pl_bolts.optimizers": bopt,
            "pl_bolts.optimizers.lr_scheduler": bsched, "pl_bolts.optimizers.lars": blars, "torchmetrics": tm,
            "models": models, "models.losses": losses, "models.losses.ntxent": ntx}


def contrastive_case(ref, out):
    torch.manual_seed(SEED)
    m = ref.SpatioTemporalContrastiveModel(dict(CT))
    fill_state_from_numpy(m.named_parameters(), SEED)
    m.projector_net[3].p = 0.0
    m.train()
    rng = np.random.default_rng(SEED + 1)
    B = CT["batch_size"]
    xs = {v: [[torch.from_numpy(rng.standard_normal((1, w)).astype(np.float32)) for w in EXPERTS] for _ in range(B)]
          for v in ("i", "j")}
    for v in ("i", "j"):
        out[f"ct_x_{v}"] = np.stack([torch.cat(e, -1)[0].numpy() for e in xs[v]])
    twin = copy.deepcopy(m)
    emb, o = twin(torch.from_numpy(out["ct_x_i"]))
    out["ct_embedding"], out["ct_output"] = emb.detach().numpy(), o.detach().numpy()
    batch = {"x_i_experts": xs["i"], "x_j_experts": xs["j"], "label": list(range(B))}
    loss = m.training_step(batch, 0)
    loss.backward()
    out["ct_loss"] = np.array(float(loss.detach()))
    for k, p in m.named_parameters():
        out[f"ct_grad:{k}"] = p.grad.numpy()
    for k in ("running_mean", "running_var", "num_batches_tracked"):
        out[f"ct_bn:{k}"] = getattr(m.encoder_net[2], k).numpy()
    out["ct_keys"] = np.array(list(m.state_dict().keys()))
    out["ct_seed"] = np.array(SEED)


def mlp_case(ref, out):
    torch.manual_seed(SEED)
    m = ref.BasicMLP({k: _View(v) for k, v in MLP.items()})
    fill_state_from_numpy(m.named_parameters(), SEED + 2)
    m.train()
    rng = np.random.default_rng(SEED + 3)
    B = MLP["batch_size"]
    x = [torch.from_numpy(rng.standard_normal((1, MLP["input_shape"])).astype(np.float32)) for _ in range(B)]
    out["mlp_x"] = np.stack([t[0].numpy() for t in x])
    out["mlp_labels"] = np.array(MLP_LABELS, dtype=np.int64)
    twin = copy.deepcopy(m)
    out["mlp_logits"] = twin(torch.from_numpy(out["mlp_x"])).detach().numpy()
    loss = m.training_step({"x_i_experts": x, "label": list(MLP_LABELS)}, 0)
    loss.backward()
    out["mlp_loss"] = np.array(float(loss.detach()))
    for k, p in m.named_parameters():
        g = p.grad.numpy()
        if g.size > 100_000:                     # fc3 / fc4 weights: the norm and the first 32 rows
            out[f"mlp_grad_norm:{k}"] = np.array(np.linalg.norm(g.astype(np.float64)))
            g = g[:32]
        out[f"mlp_grad:{k}"] = g
    for k in ("running_mean", "running_var", "num_batches_tracked"):
        out[f"mlp_bn:{k}"] = getattr(m.batchnorm, k).numpy()
    out["mlp_keys"] = np.array(list(m.state_dict().keys()))
    out["mlp_seed"] = np.array(SEED + 2)


def main():
    mods = _stand_ins()
    saved = {k: sys.modules.get(k) for k in mods}
    sys.modules.update(mods)
    try:
        ct = _load("ref_contrastivemodel", os.path.join(REF, "contrastivemodel.py"))
        mlp = _load("ref_basicmlp", os.path.join(REF, "basicmlp.py"))
    finally:
        for k, v in saved.items():
            if v is None:
                sys.modules.pop(k, None)
            else:
                sys.modules[k] = v
    out = {}
    contrastive_case(ct, out)
    mlp_case(mlp, out)
    np.savez_compressed(OUT, **out)
    print(f"contrastive_mlp: ok ({os.path.getsize(OUT)} bytes)")


if __name__ == "__main__":
    main()
