"""JointViViT on the device at the configuration of tests/golden/joint_vivit.npz: logits, loss and every gradient against
the float64 result of the imported reference modules, under the project's standing parity rule -- a 16-bit run deviates
by at most 2 x the reference's OWN deviation of that type on the same inputs (stored in the fixture per quantity), the
fp32 mode by at most 1e-3 -- and the routes its attention takes: the streamed kernels in the dense layers at 769 tokens,
the resident ones at 385."""
import pytest
import torch

from tests import joint_ref as JR
from tests.util import golden, rel_l2

pytestmark = pytest.mark.gpu

DTYPES = {"bf16": torch.bfloat16, "fp16": torch.float16}


def _model(npz, tag, dtype):
    from tests.test_joint_cpu import _model as build
    net, cfg, pool, pt = build(npz, tag, compute_dtype=dtype)
    return net.cuda().train(), cfg


def _record_routes(monkeypatch):
    """[(route, Lq, Lk, plan or None)] of every attention forward / backward the model's blocks launch"""
    from dvt_amd import ops
    calls = []

    def wrap(name, route):
        inner = getattr(ops, name)

        def f(q, k, v, o, *a, **kw):
            plan = ops.attention_long_plan(q, k, v, o, bwd=name.endswith("bwd")) if route == "long" else None
            calls.append((name, q.shape[2], k.shape[2], plan))
            return inner(q, k, v, o, *a, **kw)
        monkeypatch.setattr(ops, name, f)

    for name, route in (("attention_fwd", "resident"), ("attention_bwd", "resident"), ("attention_long_fwd", "long"),
                        ("attention_long_bwd", "long")):
        wrap(name, route)
    return calls


def _step(net, npz, device):
    clip, target = JR.inputs(npz)
    clip = clip.to(device).requires_grad_(True)
    loss, logits = net.loss(clip, target.to(device))
    loss.backward()
    torch.cuda.synchronize()
    grads = {n: p.grad for n, p in net.named_parameters()}
    grads["clip"] = clip.grad
    return logits, loss, grads


@pytest.mark.parametrize("prec", list(DTYPES))
@pytest.mark.parametrize("tag", list(JR.VARIANTS))
def test_16bit_within_twice_the_references_own_deviation(device, monkeypatch, tag, prec):
    npz = golden("joint_vivit.npz")
    net, cfg = _model(npz, tag, DTYPES[prec])
    calls = _record_routes(monkeypatch)
    logits, loss, grads = _step(net, npz, device)
    assert logits.dtype == torch.float32 and torch.isfinite(logits).all()
    assert rel_l2(net(JR.inputs(npz)[0].to(device)), logits) < 1e-2                 # forward(): the unfused head, same logits
    dev = JR.deviations(npz, tag, logits, loss, grads)
    assert set(dev) == {k.split(":", 2)[2] for k in npz.files if k.startswith(f"{tag}:dev_{prec}:")}
    over = {}
    for k, e in sorted(dev.items()):
        own = float(npz[f"{tag}:dev_{prec}:{k}"])
        print(f"{tag} {prec} {k}: {e:.3e} (reference's own {own:.3e}, ratio {e / own:.2f})")
        if not e <= 2.0 * own:
            over[k] = (e, own)
    assert not over, f"beyond 2 x the reference's own {prec} deviation: {over}"

    # routes: depth - 1 dense layers (the last layer's single CLS query keeps the Q1 kernels) or depth under mean pooling
    pool, pt = JR.VARIANTS[tag]
    tokens = cfg["frames"] // pt * (cfg["image"] // cfg["patch"]) ** 2 + 1
    dense = cfg["depth"] - (1 if pool == "cls" else 0)
    long_calls = [c for c in calls if c[0].startswith("attention_long")]
    resident = [c for c in calls if not c[0].startswith("attention_long")]
    if tokens > 640:
        assert [c[0] for c in long_calls].count("attention_long_fwd") == 2 * dense          # loss + forward
        assert [c[0] for c in long_calls].count("attention_long_bwd") == dense
        for name, Lq, Lk, plan in long_calls:
            assert (Lq, Lk) == (tokens, tokens)
            assert plan.chunks == -(-tokens // plan.k_chunk) >= 2 and plan.grid == 2 * cfg["heads"] * -(-tokens // plan.q_block)
        assert all(Lq == 1 and Lk == tokens for _, Lq, Lk, _ in resident)      # the CLS query of the last layer, if unfolded
        assert len(resident) <= (3 if pool == "cls" else 0)
    else:
        assert not long_calls
        assert len([c for c in resident if c[1:3] == (tokens, tokens)]) == 3 * dense


@pytest.mark.parametrize("tag", ["cls_t1", "mean_t1"])
def test_fp32_mode_matches_the_reference(device, monkeypatch, tag):
    """fp32 keeps the generic attention kernels past 640 keys (the streamed kernels are 16-bit)"""
    npz = golden("joint_vivit.npz")
    net, cfg = _model(npz, tag, torch.float32)
    calls = _record_routes(monkeypatch)
    logits, loss, grads = _step(net, npz, device)
    dev = JR.deviations(npz, tag, logits, loss, grads)
    worst = max(dev, key=dev.get)
    print(f"{tag} fp32 worst: {worst} {dev[worst]:.3e}")
    assert dev[worst] < 1e-3, (worst, dev[worst])
    assert calls and not [c for c in calls if c[0].startswith("attention_long")]


def test_grouped_adamw_step_changes_every_parameter(device):
    from dvt_amd import optim
    from dvt_amd.dp import FlatParameters
    npz = golden("joint_vivit.npz")
    net, cfg = _model(npz, "cls_t1", torch.bfloat16)
    flat = FlatParameters(net)
    groups = optim.param_groups(net, 1e-3, 0.05, layer_decay=0.75)
    assert len({g["lr_scale"] for g in groups}) == cfg["depth"] + 2
    flat.set_param_groups(groups)
    before = {n: p.detach().clone() for n, p in net.named_parameters()}
    clip, target = JR.inputs(npz)
    flat.zero_grad()
    loss = net.loss(clip.to(device), target.to(device))[0]
    loss.backward(torch.full((), flat.loss_scale, device=device))
    flat.finish_backward()
    flat.adamw_groups_step(torch.tensor([1e-3], dtype=torch.float32, device=device))
    torch.cuda.synchronize()
    for n, p in net.named_parameters():
        assert torch.isfinite(p).all(), n
        assert not torch.equal(p, before[n]), f"{n} did not move"
