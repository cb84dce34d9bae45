"""CPU-side checks of the online probe (SSLOnlineEval / SSLEvaluator, src/callbacks/callbacks.py:147-300): the host score
functions against scikit-learn's own values (tests/golden/ssl_online.npz, written by tools/gen_golden_ssl_online.py), the
probe's module tree and state dict, the refusals, the exported entry points and the callback's log keys."""
import inspect

import numpy as np
import pytest
import torch
from torch import nn

from tests import ssl_online_ref as R
from tests.util import golden


def test_fixture_has_every_zero_division_branch_and_the_restated_counts():
    g = golden("ssl_online.npz")
    p, y, th = g["probs"], g["labels"], g["thresholds"]
    assert p.shape == y.shape == (83, 15) and list(th) == [0.0, 0.1, 0.2, 0.3, 0.4, 0.5]
    assert min(np.abs(p - np.float32(t)).min() for t in th if t > 0) >= 9e-5
    counts, support = R.sweep_counts(p, y, th)
    assert np.array_equal(counts, g["counts"]) and np.array_equal(support, g["support"])
    assert support[11] == 0                                                   # a class without support
    assert (counts[:, 0, 4] + counts[:, 1, 4] == 0).all()                     # never predicted, even at t = 0
    assert (counts[:, 0, 7] + counts[:, 1, 7] == 83).all()                    # always predicted
    assert (y.sum(1) == 0).sum() >= 3                                         # rows without labels


def test_host_scores_reproduce_sklearn_from_the_counts():
    from dvt_amd.metrics import ONLINE_THRESHOLDS, online_scalars_from_counts
    g = golden("ssl_online.npz")
    got = online_scalars_from_counts(torch.from_numpy(g["counts"]), torch.from_numpy(g["support"]), g["probs"].shape[0])
    assert list(got) == list(g["keys"]) and len(got) == 24
    assert list(ONLINE_THRESHOLDS) == list(g["thresholds"])
    assert "val/online/f1@0.0" in got and "val/online/avg_precision@0.5" in got
    assert np.abs(np.array([got[k] for k in g["keys"]]) - g["scalars"]).max() < 1e-12


def test_evaluator_module_tree_and_state_dict():
    from dvt_amd.models.evaluator import SSLEvaluator
    import dvt_amd.models as M
    assert M.SSLEvaluator is SSLEvaluator
    assert list(inspect.signature(SSLEvaluator.__init__).parameters)[1:] == ["n_input", "n_classes", "n_hidden", "p"]
    e = SSLEvaluator(305, 15)
    kinds = [type(m) for m in e.block_forward]
    assert kinds == [nn.Flatten, nn.Dropout, nn.Linear, nn.BatchNorm1d, nn.ReLU, nn.Dropout, nn.Linear]
    assert e.block_forward[1].p == e.block_forward[5].p == 0.1 and e.block_forward[4].inplace
    sd = e.state_dict()
    assert list(sd) == ["block_forward.2.weight", "block_forward.3.weight", "block_forward.3.bias",
                        "block_forward.3.running_mean", "block_forward.3.running_var",
                        "block_forward.3.num_batches_tracked", "block_forward.6.weight", "block_forward.6.bias"]
    assert sd["block_forward.2.weight"].shape == (512, 305) and sd["block_forward.6.weight"].shape == (15, 512)
    assert sd["block_forward.6.bias"].shape == (15,) and sd["block_forward.3.running_var"].shape == (512,)
    assert all(p.dtype == torch.float32 for p in e.parameters())
    assert SSLEvaluator(40, 19, n_hidden=32, p=0.0).block_forward[2].weight.shape == (32, 40)


def test_evaluator_refusals():
    from dvt_amd.models.evaluator import SSLEvaluator
    with pytest.raises(NotImplementedError, match="n_hidden=None"):
        SSLEvaluator(305, 15, n_hidden=None)
    for kw in (dict(n_input=4097, n_classes=15), dict(n_input=305, n_classes=33), dict(n_input=305, n_classes=15, n_hidden=500),
               dict(n_input=305, n_classes=15, n_hidden=4096)):
        with pytest.raises(NotImplementedError, match="4096"):
            SSLEvaluator(**kw)
    with pytest.raises(RuntimeError, match="no CPU path"):
        SSLEvaluator(40, 19, n_hidden=32).eval()(torch.randn(4, 40))


def test_library_range_and_argument_checks_without_gpu():
    import dvt_amd
    from dvt_amd import _lib
    lib = _lib.load()
    for name in ("dvt_probe_supported", "dvt_probe_workspace_bytes", "dvt_probe_fwd", "dvt_probe_loss",
                 "dvt_probe_bwd_step", "dvt_multilabel_sweep_counts"):
        assert name in _lib.SIGNATURES, name
    ok = [(256, 305, 512, 15), (7, 40, 32, 19), (1024, 2048, 512, 15), (2, 4096, 2048, 32), (1, 1, 16, 1)]
    for dt in (_lib.F32, _lib.BF16, _lib.F16):
        assert all(lib.dvt_probe_supported(*s, dt) == 1 for s in ok)
    bad = [(1025, 305, 512, 15), (256, 4097, 512, 15), (256, 305, 520, 15), (256, 305, 2064, 15), (256, 305, 512, 33),
           (0, 305, 512, 15)]
    assert all(lib.dvt_probe_supported(*s, _lib.BF16) == 0 for s in bad)
    assert lib.dvt_probe_supported(256, 305, 512, 15, 7) == 0
    assert lib.dvt_probe_workspace_bytes(256, 512, 15) == 4 * 32 * 256 * 15
    d = _lib.STRUCTS["dvt_probe_desc"]()
    d.B, d.D, d.H, d.C, d.dtype, d.training = 1, 305, 512, 15, _lib.F32, 1          # B = 1 in training: refused as torch does
    import ctypes
    assert lib.dvt_probe_fwd(ctypes.byref(d), None) == -1 and b"more than 1 value per channel" in lib.dvt_last_error()
    d.B = 2000
    assert lib.dvt_probe_bwd_step(ctypes.byref(d), None) != 0 and b"outside the probe kernels' range" in lib.dvt_last_error()
    assert lib.dvt_multilabel_sweep_counts(None, None, 4, 4, None, 6, None, None, None) == -1


class _Stub(nn.Module):
    """A module with the attributes the callback touches; its forward is never reached."""

    def __init__(self):
        super().__init__()
        self.w = nn.Parameter(torch.zeros(1))
        self.running_logits, self.running_labels, self.logged = [], [], {}

    def log(self, name, value, **kw):
        self.logged[name] = value

    def forward(self, x):
        raise AssertionError("the stub's forward must not be reached")


def test_callback_surface_log_keys_and_accumulator_reset(monkeypatch):
    from dvt_amd import metrics
    from dvt_amd.models.evaluator import SSLEvaluator
    assert list(inspect.signature(metrics.SSLOnlineEval.__init__).parameters)[1:] == ["drop_p", "z_dim", "num_classes", "model",
                                                                                 "group", "zero_grad"]
    cb = metrics.SSLOnlineEval(drop_p=0.2, z_dim=40, num_classes=15)
    assert cb.lr == 0.005 and cb.zero_grad is False
    m = _Stub()
    cb.on_pretrain_routine_start(None, m)
    assert isinstance(m.non_linear_evaluator, SSLEvaluator) and m.non_linear_evaluator.block_forward[1].p == 0.2
    assert m.non_linear_evaluator.block_forward[2].weight.shape == (512, 40)
    assert cb.optimizer["lr"] == 0.005 and len(cb.optimizer["params"]) == 5
    g = golden("ssl_online.npz")
    probs, labels = torch.from_numpy(g["probs"]), torch.from_numpy(g["labels"])
    m.running_logits, m.running_labels = [probs[:40], probs[40:]], [labels[:40], labels[40:]]
    # counts injected in place of the device launch
    monkeypatch.setattr(metrics.ops, "multilabel_sweep_counts",
                        lambda p, y, th: (torch.from_numpy(g["counts"]), torch.from_numpy(g["support"])))
    tables = []
    m.logger = type("L", (), {"experiment": type("E", (), {"log": staticmethod(tables.append)})()})()
    scalars, rows = cb.on_validation_epoch_end(None, m)
    assert list(scalars) == list(g["keys"]) and set(scalars) <= set(m.logged) and len(scalars) == 24
    assert np.abs(np.array([m.logged[k] for k in g["keys"]]) - g["scalars"]).max() < 1e-12
    assert m.running_logits == [] and m.running_labels == []
    assert len(rows) == 20 and tables == [{"table": rows}]
    truth0 = [metrics.ONLINE_TARGET_NAMES[i] for i in range(15) if g["labels"][0, i]]
    guess0 = [metrics.ONLINE_TARGET_NAMES[i] for i in range(15) if g["probs"][0, i] > np.float32(0.3)]
    assert rows[0] == (truth0, guess0)
    assert len(metrics.ONLINE_TARGET_NAMES) == 15 and cb.translate_labels([0, 1, 0]) == ["Adventure"]
    # a short epoch: the table shrinks instead of failing
    m.running_logits, m.running_labels = [probs[:7]], [labels[:7]]
    del m.logger
    _, rows = cb.on_shared_end(m, "val")
    assert len(rows) == 7
