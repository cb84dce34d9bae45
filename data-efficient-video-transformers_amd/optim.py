"""HIP-backed optimizers behind the ``torch.optim.Optimizer`` interface that Lightning's trainer drives
(``configure_optimizers`` of the reference: frame_transformer.py:123-134, transformer.py:58-61).

Per-parameter launches of the fused update kernels (``dvt_adamw_step`` / ``dvt_adam_step_dev`` / ``dvt_sgd_step`` /
``dvt_adagrad_step``), and ``LARS`` with one ``dvt_lars_step`` per parameter group; a model wrapped in
``dp.FlatParameters`` should use its one-launch ``adamw_step`` / ``adam_step`` / ``sgd_step`` / ``adagrad_step`` /
``lars_step`` instead.  State names match torch's
(``exp_avg``, ``exp_avg_sq``, ``momentum_buffer``, ``sum``, ``step``) so optimizer state dicts
written by the reference load unchanged.
"""
from __future__ import annotations

import torch

from . import ops


def _grad32(p):
    g = p.grad
    if g is None:
        return None
    sink = getattr(p, "_dvt_sink", None)
    if sink is not None and (sink.fresh or sink.unwritten):
        return None        # a FlatParameters view nobody wrote a gradient into: torch would see grad None and skip it
    if g.dtype != torch.float32 or not g.is_contiguous():
        raise RuntimeError("optimizer expects contiguous fp32 gradients (master weights are fp32)")
    return g


def _zeros_like(p):
    return torch.zeros_like(p, memory_format=torch.contiguous_format)


_clip_tables = {}          # (gradient data pointers) -> ops.LarsTable over them; one entry per set, as LARS caches its table


def clip_grad_norm_(parameters, max_norm, norm_type=2.0, error_if_nonfinite=False) -> torch.Tensor:
    """torch.nn.utils.clip_grad_norm_ (Lightning's ``gradient_clip_val``) for the per-parameter optimizers of this module:
    ONE norm over the gradients of all ``parameters`` that have one, then ``g *= min(1, max_norm / (norm + 1e-6))`` in
    place, in two launches (``dvt_grad_clip``).  "Has a gradient" is the optimizers' rule (``_grad32``): a
    ``FlatParameters`` view nobody wrote is left out, like ``grad is None``.  Returns the norm before clipping as a device
    fp32 scalar; no host synchronisation.  The segment table is cached on the set of gradient addresses and rebuilt when
    it changes (which may not happen inside a hipGraph capture).  ``norm_type``: 2 or inf.  ``error_if_nonfinite=True``
    needs a host read of the norm and raises NotImplementedError; deviation from torch: a non-finite norm leaves the
    gradients as they are instead of spreading NaN.  A model wrapped in ``dp.FlatParameters`` should call its
    ``clip_grad_norm_`` (one segment, and the loss scale)."""
    if error_if_nonfinite:
        raise NotImplementedError("error_if_nonfinite=True needs a host read of the norm; check the returned scalar instead")
    ops.norm_kind(norm_type)                  # NotImplementedError for any other norm
    if isinstance(parameters, torch.Tensor):
        parameters = [parameters]
    grads = [g for p in parameters for g in (_grad32(p),) if g is not None and g.numel() > 0]
    if not grads:
        return torch.zeros(1, dtype=torch.float32)
    sig = tuple(g.data_ptr() for g in grads) + tuple(g.numel() for g in grads)
    table = _clip_tables.get(sig)
    if table is None:
        if _capturing():
            raise RuntimeError("the set of parameters with a gradient, or a gradient's address, changed inside a hipGraph "
                               "capture; run a warm-up step first and keep the gradient tensors (zero_grad(set_to_none=False))")
        if len(_clip_tables) >= 8:            # gradients that torch allocates anew every step: do not hoard their tables
            _clip_tables.clear()
        table = _clip_tables[sig] = ops.grad_table(grads)
    return ops.grad_clip_(table, max_norm, norm_type)


def param_groups(module, lr, weight_decay, *, layer_decay=None, no_weight_decay=None, layer_id=None, num_layers=None):
    """The fine-tuning grouping of MAE's ``param_groups_lrd`` (also VideoMAE, DeiT, timm): a list of group dicts
    ``{"params", "names", "weight_decay", "lr_scale", "lr": lr * lr_scale}`` that ``AdamW`` of this module and
    ``FlatParameters.set_param_groups`` both accept.

    A parameter is NOT decayed if ``p.ndim <= 1``, its name ends in ``.bias`` or its name is in ``no_weight_decay``
    (default: ``module.no_weight_decay()`` where the module has it).  With ``layer_decay`` the rate shrinks geometrically
    from the head down: ``lr_scale = layer_decay ** (num_layers - layer_id(name))``; ``layer_id`` / ``num_layers`` default
    to ``module.layer_id`` / ``module.num_lr_layers``.  Without it every scale is 1 and there are exactly two groups.
    Groups are ordered by (layer id, decayed first); parameters keep their registration order inside a group."""
    if no_weight_decay is None:
        no_weight_decay = module.no_weight_decay() if hasattr(module, "no_weight_decay") else ()
    no_weight_decay = set(no_weight_decay)
    if layer_decay is not None:
        layer_id = layer_id if layer_id is not None else getattr(module, "layer_id", None)
        num_layers = num_layers if num_layers is not None else getattr(module, "num_lr_layers", None)
        if layer_id is None or num_layers is None:
            raise ValueError("param_groups: layer_decay needs layer_id and num_layers (the module has no layer_id / "
                             "num_lr_layers of its own)")
    groups, seen = {}, set()
    for name, p in module.named_parameters():
        if not p.requires_grad or id(p) in seen:
            continue
        seen.add(id(p))
        decayed = not (p.ndim <= 1 or name.endswith(".bias") or name in no_weight_decay)
        layer = int(layer_id(name)) if layer_decay is not None else 0
        scale = float(layer_decay) ** (num_layers - layer) if layer_decay is not None else 1.0
        g = groups.setdefault((layer, not decayed), {"params": [], "names": [], "weight_decay": weight_decay if decayed else 0.0,
                                                     "lr_scale": scale, "lr": lr * scale})
        g["params"].append(p)
        g["names"].append(name)
    return [groups[k] for k in sorted(groups)]


class _Base(torch.optim.Optimizer):
    """The one ``step()``: closure, groups, parameters with a gradient.  A subclass supplies ``_init_state`` (create what is
    missing from a parameter's state) and ``_update`` (its one kernel call)."""

    def _invalidate(self, p):
        sink = getattr(p, "_dvt_sink", None)
        if sink is not None:                      # parameters were updated behind a FlatParameters mirror
            sink.owner.invalidate_compute_copy()

    def _begin_step(self):
        pass

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._begin_step()
        for i, grp in enumerate(self.param_groups):
            for p in grp["params"]:
                g = _grad32(p)
                if g is None:
                    continue
                st = self.state[p]
                self._init_state(st, p, grp)
                self._update(p, g, st, grp, i)
                self._invalidate(p)
        return loss


class AdamW(_Base):
    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2):
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay))

    def _init_state(self, st, p, grp):
        if not st:
            st["step"] = 0
            st["exp_avg"] = _zeros_like(p)
            st["exp_avg_sq"] = _zeros_like(p)

    def _update(self, p, g, st, grp, i):
        st["step"] = int(st["step"]) + 1
        ops.adamw_step_(p.data, g, st["exp_avg"], st["exp_avg_sq"], lr=grp["lr"], beta1=grp["betas"][0],
                        beta2=grp["betas"][1], eps=grp["eps"], weight_decay=grp["weight_decay"], step=st["step"])


class _DeviceLR(_Base):
    """One device fp32 LR scalar per parameter group (``lr_dev(i)``) that the group's updates read, so that a step captured
    in a hipGraph follows a new rate written by ``sync_lr()`` (which ``lr_scheduler.LinearWarmupCosineAnnealingLR.step``
    calls)."""

    def _init_lr_dev(self):
        self._lr_dev = []
        self._lr_host = []
        for grp in self.param_groups:
            dev = grp["params"][0].device if grp["params"] else torch.device("cpu")
            self._lr_dev.append(torch.full((1,), float(grp["lr"]), dtype=torch.float32, device=dev))
            self._lr_host.append(float(grp["lr"]))

    def lr_dev(self, group: int = 0) -> torch.Tensor:
        """The device fp32 scalar the updates of param group ``group`` read their learning rate from."""
        return self._lr_dev[group]

    def sync_lr(self) -> None:
        """Write each group's ``lr`` into its device scalar where it changed (a fill launch on the current stream)."""
        for i, grp in enumerate(self.param_groups):
            lr = float(grp["lr"])
            if lr != self._lr_host[i]:
                self._lr_dev[i].fill_(lr)
                self._lr_host[i] = lr

    def _begin_step(self):
        if not _capturing():              # a rate set by hand; inside a capture the scalar is written from outside
            self.sync_lr()


def _capturing() -> bool:
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


class Adam(_DeviceLR):
    """torch.optim.Adam (amsgrad off) with coupled L2 weight decay (``g += weight_decay * p`` before the moments):
    contrastivemodel.py:64 and basicmlp.py:49.  The optimizer owns one device fp32 LR scalar per parameter group
    (``lr_dev(i)``) that every update reads, and one device step counter per parameter (``state["step"]``, int64[2]:
    steps taken, launch ticket), so ``step()`` has no host synchronisation and can be captured in a hipGraph; a captured
    step follows a new rate written by ``sync_lr()`` (which ``lr_scheduler.LinearWarmupCosineAnnealingLR.step`` calls)."""

    def __init__(self, params, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, amsgrad=False):
        if amsgrad:
            raise NotImplementedError("Adam(amsgrad=True) has no HIP kernel")
        super().__init__(params, dict(lr=lr, betas=betas, eps=eps, weight_decay=weight_decay, amsgrad=False))
        self._init_lr_dev()

    def _init_state(self, st, p, grp):
        if not st:
            st["step"] = torch.zeros(2, dtype=torch.int64, device=p.device)
            st["exp_avg"] = _zeros_like(p)
            st["exp_avg_sq"] = _zeros_like(p)

    def _update(self, p, g, st, grp, i):
        ops.adam_step_dev_(p.data, g, st["exp_avg"], st["exp_avg_sq"], st["step"], self._lr_dev[i],
                           beta1=grp["betas"][0], beta2=grp["betas"][1], eps=grp["eps"],
                           weight_decay=grp["weight_decay"])


class SGD(_Base):
    def __init__(self, params, lr=1e-3, momentum=0.0, weight_decay=0.0):
        super().__init__(params, dict(lr=lr, momentum=momentum, weight_decay=weight_decay))

    def _init_state(self, st, p, grp):
        if grp["momentum"] != 0 and "momentum_buffer" not in st:
            st["momentum_buffer"] = _zeros_like(p)

    def _update(self, p, g, st, grp, i):
        ops.sgd_step_(p.data, g, st.get("momentum_buffer"), lr=grp["lr"], momentum=grp["momentum"],
                      weight_decay=grp["weight_decay"])


class Adagrad(_Base):
    def __init__(self, params, lr=1e-2, lr_decay=0.0, weight_decay=0.0, eps=1e-10):
        super().__init__(params, dict(lr=lr, lr_decay=lr_decay, weight_decay=weight_decay, eps=eps))

    def _init_state(self, st, p, grp):
        if not st:
            st["step"] = 0
            st["sum"] = _zeros_like(p)

    def _update(self, p, g, st, grp, i):
        st["step"] = int(st["step"]) + 1
        ops.adagrad_step_(p.data, g, st["sum"], lr=grp["lr"], lr_decay=grp["lr_decay"], eps=grp["eps"],
                          weight_decay=grp["weight_decay"], step=st["step"])


class LARS(_DeviceLR):
    """pl_bolts' ``LARS`` (layer-wise adaptive rate scaling: contrastivemodel.py:8, :64-70), per parameter with a gradient:

        d = g
        if weight_decay != 0 and |p| != 0 and |g| != 0:
            d = trust_coefficient |p| / (|g| + weight_decay |p| + eps) * (g + weight_decay p)
        if momentum != 0:
            buf = d on the first step, momentum buf + (1 - dampening) d afterwards
            d = d + momentum buf if nesterov else buf
        p = p - lr d

    so ``weight_decay == 0`` is plain momentum SGD, and a zero norm drops the decay term too.  One ``dvt_lars_step`` (two
    launches: norms, update) per parameter group and step, over a device table of the group's parameters that have a
    gradient; the table is rebuilt only when that set changes.  Gradient tensors that torch allocates anew every step
    (``zero_grad(set_to_none=True)``, its default) cost one small asynchronous copy of the table's rows per step, which
    refreshes the gradient pointers and nothing else; gradients kept in place (``set_to_none=False``) cost nothing.
    Neither may happen inside a hipGraph capture, whose launches hold the addresses they were captured with.
    The learning rate is read from ``lr_dev(i)`` as in ``Adam``; no host synchronisation.  State: ``momentum_buffer`` per
    parameter, as torch's SGD and pl_bolts name it.

    One deviation: "the first step" is the GROUP's (one device counter per group), where pl_bolts looks at each parameter's
    own state.  A parameter that receives its first gradient in a later step starts from a zero buffer, buf =
    (1 - dampening) d instead of d; the two agree whenever dampening == 0 or every parameter has a gradient from the first
    step on.  Under data parallelism the norms are those of the gradient the step sees, i.e. the all-reduced one when the
    step follows ``FlatParameters.finish_backward``."""

    def __init__(self, params, lr, momentum=0, dampening=0, weight_decay=0, nesterov=False, trust_coefficient=0.001,
                 eps=1e-8):
        if lr < 0.0:
            raise ValueError(f"Invalid learning rate: {lr}")
        if momentum < 0.0:
            raise ValueError(f"Invalid momentum value: {momentum}")
        if weight_decay < 0.0:
            raise ValueError(f"Invalid weight_decay value: {weight_decay}")
        if nesterov and (momentum <= 0 or dampening != 0):
            raise ValueError("Nesterov momentum requires a momentum and zero dampening")
        super().__init__(params, dict(lr=lr, momentum=momentum, dampening=dampening, weight_decay=weight_decay,
                                      nesterov=nesterov, trust_coefficient=trust_coefficient, eps=eps))
        self._init_lr_dev()
        self._tables = {}          # group index -> (signature, ops.LarsTable)
        self._step_dev = {}        # group index -> int64[2] on the device: steps taken, launch ticket

    def __setstate__(self, state):
        super().__setstate__(state)
        for grp in self.param_groups:
            grp.setdefault("nesterov", False)

    def load_state_dict(self, state_dict):
        super().load_state_dict(state_dict)
        self._tables, self._step_dev = {}, {}      # the loaded buffers are other tensors; groups that hold one have stepped

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        self._begin_step()
        for i, grp in enumerate(self.param_groups):
            live = [(p, g) for p in grp["params"] for g in (_grad32(p),) if g is not None and p.numel() > 0]
            if not live:
                continue
            mom = grp["momentum"] != 0
            if i not in self._step_dev:
                resumed = any("momentum_buffer" in self.state[p] for p, _ in live)
                self._step_dev[i] = torch.tensor([int(resumed), 0], dtype=torch.int64, device=live[0][0].device)
            sig = tuple(p.data_ptr() for p, _ in live) + (mom, grp["weight_decay"])
            grads = tuple(g.data_ptr() for _, g in live)
            cached = self._tables.get(i)
            if cached is None or cached[0] != sig or cached[1].grad_ptrs() != grads:
                if _capturing():
                    raise RuntimeError("the set of parameters with a gradient, or a gradient's address, changed inside a "
                                       "hipGraph capture; run the warm-up steps with the same model mode as the captured "
                                       "step and keep the gradient tensors (zero_grad(set_to_none=False))")
                if cached is not None and cached[0] == sig:
                    cached[1].set_grads(g for _, g in live)        # fresh gradient tensors: only their pointers change
                else:
                    for p, _ in live:
                        if mom and "momentum_buffer" not in self.state[p]:
                            self.state[p]["momentum_buffer"] = _zeros_like(p)
                    cached = (sig, ops.lars_table([(p.data, g, self.state[p].get("momentum_buffer") if mom else None,
                                                    None, grp["weight_decay"]) for p, g in live]))
                    self._tables[i] = cached
            ops.lars_step_(cached[1], self._lr_dev[i], self._step_dev[i], momentum=grp["momentum"],
                           dampening=grp["dampening"], nesterov=grp["nesterov"],
                           trust_coefficient=grp["trust_coefficient"], eps=grp["eps"])
            for p, _ in live:
                self._invalidate(p)
        return loss
