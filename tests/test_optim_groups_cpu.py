"""Grouped AdamW and weight EMA without a GPU: the two entry points of csrc/optim_groups.hip in include/dvt_hip.h and the
derived binding with every refusal message, ``optim.param_groups`` on the small ViViT against a hand-written table,
``FlatParameters.set_param_groups`` on CPU tensors, and tests/optim_groups_ref.py against torch.optim.AdamW and timm's EMA
formula."""
import ctypes as C
import math

import pytest
import torch
from torch import nn

from tests import optim_groups_ref as G
from tests import optim_ref as O


def _vivit():
    from dvt_amd.models.vit import ViViT
    torch.manual_seed(3)
    return ViViT(64, 16, 19, 4, dim=128, depth=2, heads=2)


# ---------------------------------------------------------------- header, binding, argument checks
def test_entry_points_exist_and_refuse_before_any_hip_call():
    import dvt_amd
    from dvt_amd import _lib
    lib = dvt_amd._lib.load()
    assert lib.dvt_version() == 5 and _lib.ABI_VERSION == 5                  # entry points were only added
    res, args = _lib.SIGNATURES["dvt_adamw_groups_step"]
    assert res is C.c_int and len(args) == 19 and args[4] is C.c_int64 and args[11] is C.c_int and args[15] is C.c_int
    res, args = _lib.SIGNATURES["dvt_ema_update"]
    assert res is C.c_int and len(args) == 5 and args[2] is C.c_int64
    with open(_lib.HEADER_PATH) as fh:
        text = fh.read()
    assert "int dvt_adamw_groups_step(" in text and "int dvt_ema_update(" in text

    p, odd, bf16, f32 = 256, 260, _lib.BF16, _lib.F32

    def step(param=p, grad=p, m=p, v=p, n=64, lr=p, group64=p, table=p, ngroups=3, step_dev=p, skip=None, mirror=None,
             mdt=0, ema=None, decay=None):
        return lib.dvt_adamw_groups_step(param, grad, m, v, n, lr, 0.9, 0.999, 1e-8, group64, table, ngroups, step_dev, skip,
                                         mirror, mdt, ema, decay, None)
    bad, aligned, mir = "bad arguments", "buffers must be 16-byte aligned", "mirror must be bf16 / f16 and 8-byte aligned"
    checks = [(bad, dict(param=None)), (bad, dict(grad=None)), (bad, dict(m=None)), (bad, dict(v=None)), (bad, dict(lr=None)),
              (bad, dict(group64=None)), (bad, dict(table=None)), (bad, dict(step_dev=None)), (bad, dict(n=-1)),
              ("ngroups must be in 1 .. 255", dict(ngroups=0)), ("ngroups must be in 1 .. 255", dict(ngroups=256)),
              ("ngroups must be in 1 .. 255", dict(ngroups=-1)),
              ("ema needs ema_decay_dev", dict(ema=p)),
              (aligned, dict(param=odd)), (aligned, dict(grad=odd)), (aligned, dict(m=odd)), (aligned, dict(v=odd)),
              (aligned, dict(ema=odd, decay=p)),
              ("group_table must be 8-byte aligned", dict(table=odd)),
              (mir, dict(mirror=odd, mdt=bf16)), (mir, dict(mirror=p, mdt=f32)), (mir, dict(mirror=p, mdt=7))]
    for msg, kw in checks:
        assert step(**kw) == -1, kw
        assert f"dvt_adamw_groups_step: {msg}".encode() in lib.dvt_last_error(), (kw, lib.dvt_last_error())
    assert step(n=0, param=None, grad=None, m=None, v=None, ngroups=0) == 0          # n == 0 is a no-op whatever else is handed

    for msg, a in [(bad, (None, p, 64, p)), (bad, (p, None, 64, p)), (bad, (p, p, 64, None)), (bad, (p, p, -1, p)),
                   (aligned, (odd, p, 64, p)), (aligned, (p, odd, 64, p))]:
        assert lib.dvt_ema_update(*a, None) == -1, a
        assert f"dvt_ema_update: {msg}".encode() in lib.dvt_last_error(), a
    assert lib.dvt_ema_update(None, None, 0, None, None) == 0


def test_group_table_is_validated_on_the_host():
    from dvt_amd import ops
    m = torch.tensor([0, 1, 2, 1], dtype=torch.uint8)
    with pytest.raises(ValueError, match="map byte 2 at block 2 is not below ngroups = 2"):
        ops.adamw_group_table(m, [1.0, 0.5], [0.1, 0.0])
    for k in (0, 256):
        with pytest.raises(ValueError, match="ngroups must be in 1 .. 255"):
            ops.adamw_group_table(torch.zeros(4, dtype=torch.uint8), [1.0] * k, [0.0] * k)
    with pytest.raises(ValueError, match="2 lr_scales for 1 weight_decays"):
        ops.adamw_group_table(m, [1.0, 0.5], [0.1])
    with pytest.raises(TypeError, match="uint8"):
        ops.adamw_group_table(m.to(torch.int64), [1.0, 0.5, 0.25], [0.0] * 3)


# ---------------------------------------------------------------- optim.param_groups on the small ViViT
def test_param_groups_equal_the_hand_written_table():
    from dvt_amd import optim
    net = _vivit()
    assert net.num_lr_layers == 5 and net.no_weight_decay() == {"pos_embedding", "space_token", "temporal_token"}
    lr, wd = 1e-3, 0.05
    groups = optim.param_groups(net, lr, wd, layer_decay=0.5)
    # the hand-written table: prefix -> layer id (Ds = Dt = 2)
    layer = {"to_patch_embedding.": 0, "pos_embedding": 0, "space_token": 0, "space_transformer.layers.0.": 1,
             "space_transformer.layers.1.": 2, "space_transformer.norm.": 2, "temporal_token": 3,
             "temporal_transformer.layers.0.": 3, "temporal_transformer.layers.1.": 4, "temporal_transformer.norm.": 5,
             "mlp_head.": 5}
    named = dict(net.named_parameters())
    want_layer = {}
    for name in named:
        hits = [v for k, v in layer.items() if name == k or (k.endswith(".") and name.startswith(k))]
        assert len(hits) == 1, name
        want_layer[name] = hits[0]
        assert net.layer_id(name) == hits[0], name
    assert set(want_layer.values()) == {0, 1, 2, 3, 4, 5}
    seen = {}
    for g in groups:
        assert set(g) == {"params", "names", "weight_decay", "lr_scale", "lr"}
        assert g["lr"] == lr * g["lr_scale"] and len(g["params"]) == len(g["names"]) > 0
        for name, p in zip(g["names"], g["params"]):
            assert p is named[name] and name not in seen
            seen[name] = g
            assert g["lr_scale"] == 0.5 ** (5 - want_layer[name]), name
    assert set(seen) == set(named)                                               # every parameter is in one group
    assert sorted({g["lr_scale"] for g in groups}) == [2.0 ** -k for k in range(5, -1, -1)]
    not_decayed = {n for n, g in seen.items() if g["weight_decay"] == 0.0}
    assert all(g["weight_decay"] in (0.0, wd) for g in groups)
    assert not_decayed == {n for n, p in named.items() if p.ndim <= 1} | {"pos_embedding", "space_token", "temporal_token"}
    assert all(n.endswith(".weight") and named[n].ndim == 2 for n in set(named) - not_decayed)
    # ordered by (layer id, decayed first)
    keys = [(want_layer[g["names"][0]], g["weight_decay"] == 0.0) for g in groups]
    assert keys == sorted(keys) and len(set(keys)) == len(keys) == 12
    with pytest.raises(KeyError):
        net.layer_id("space_transformer.layers.2.0.norm.weight")
    with pytest.raises(KeyError):
        net.layer_id("decoder_pred.weight")


def test_param_groups_without_layer_decay_and_on_a_foreign_module():
    from dvt_amd import optim
    net = _vivit()
    groups = optim.param_groups(net, 1e-3, 0.05)
    assert len(groups) == 2 and [g["weight_decay"] for g in groups] == [0.05, 0.0]
    assert all(g["lr_scale"] == 1.0 and g["lr"] == 1e-3 for g in groups)
    assert sum(len(g["params"]) for g in groups) == len(list(net.parameters()))
    assert "pos_embedding" in groups[1]["names"] and "to_patch_embedding.1.weight" in groups[0]["names"]
    foreign = nn.Sequential(nn.Linear(4, 4), nn.LayerNorm(4))
    two = optim.param_groups(foreign, 0.1, 0.01)
    assert [g["names"] for g in two] == [["0.weight"], ["0.bias", "1.weight", "1.bias"]]
    with pytest.raises(ValueError, match="layer_id"):
        optim.param_groups(foreign, 0.1, 0.01, layer_decay=0.75)
    three = optim.param_groups(foreign, 0.1, 0.01, layer_decay=0.5, layer_id=lambda n: int(n[0]), num_layers=1)
    assert [(g["lr_scale"], g["weight_decay"], g["names"]) for g in three] == [
        (0.5, 0.01, ["0.weight"]), (0.5, 0.0, ["0.bias"]), (1.0, 0.0, ["1.weight", "1.bias"])]
    # the per-tensor optimizer takes the same groups
    opt = optim.AdamW(three, lr=0.1)
    assert [g["lr"] for g in opt.param_groups] == [0.05, 0.05, 0.1]


def test_mae_no_weight_decay_is_the_encoders_set_prefixed():
    from dvt_amd import optim
    from dvt_amd.models.mae import MaskedClipAutoencoder
    mae = MaskedClipAutoencoder(_vivit(), decoder_dim=64, decoder_depth=1, decoder_heads=2, decoder_dim_head=32)
    assert mae.no_weight_decay() == {"encoder.pos_embedding", "encoder.space_token", "encoder.temporal_token", "mask_token",
                                     "decoder_pos_embedding"}
    assert mae.no_weight_decay() <= set(dict(mae.named_parameters()))
    decayed, rest = optim.param_groups(mae, 1e-3, 0.05)
    assert all(p.ndim == 2 for p in decayed["params"]) and mae.no_weight_decay() <= set(rest["names"])


# ---------------------------------------------------------------- FlatParameters.set_param_groups on CPU tensors
def test_set_param_groups_builds_the_block_map():
    from dvt_amd import optim
    from dvt_amd.dp import FlatParameters
    net = _vivit()
    flat = FlatParameters(net, compute_dtype=None)
    groups = optim.param_groups(net, 1e-3, 0.05, layer_decay=0.75)
    with pytest.raises(RuntimeError, match="set_param_groups first"):
        flat.adamw_groups_step(1e-3)
    flat.set_param_groups(groups)
    m = flat.group64
    assert m.dtype == torch.uint8 and m.numel() * 64 == flat.total
    group_of = {id(p): gi for gi, g in enumerate(groups) for p in g["params"]}
    covered = torch.zeros(m.numel(), dtype=torch.bool)
    for p, off in zip(flat.params, flat.offsets):
        assert off % 64 == 0
        lo, hi = off // 64, (off + p.numel() + 63) // 64
        assert bool((m[lo:hi] == group_of[id(p)]).all())
        covered[lo:hi] = True
    assert bool(covered.all())                                   # this layout pads inside a parameter's last block only
    assert flat.group_hyper == [(g["lr_scale"], g["weight_decay"]) for g in groups]
    # padding blocks of their own take group 0: a layout with a gap
    lin = nn.Linear(3, 2)
    f2 = FlatParameters(lin, compute_dtype=None)
    f2.total += 64                                               # a trailing block no parameter owns
    f2.set_param_groups([{"params": [lin.bias], "weight_decay": 0.0}, {"params": [lin.weight], "weight_decay": 0.1, "lr_scale": 0.5}])
    assert f2.group64.tolist() == [1, 0, 0] and f2.group_hyper == [(1.0, 0.0), (0.5, 0.1)]
    # a missing and a doubled parameter
    with pytest.raises(ValueError, match="is in no group"):
        flat.set_param_groups([dict(g, params=g["params"][1:], names=g["names"][1:]) if i == 0 else g
                               for i, g in enumerate(groups)])
    first = groups[0]["names"][0]
    with pytest.raises(ValueError, match=f"parameter {first} is in group 0 and in group 1"):
        flat.set_param_groups([dict(g, params=g["params"] + groups[0]["params"][:1], names=g["names"] + [first])
                               if i == 1 else g for i, g in enumerate(groups)])
    with pytest.raises(ValueError, match="not a trainable parameter of the module"):
        flat.set_param_groups(groups + [{"params": [nn.Parameter(torch.zeros(3))]}])
    with pytest.raises(RuntimeError, match="no CPU path"):
        flat.adamw_groups_step(1e-3)


def test_ema_state_travels_and_loss_scaling_is_refused_by_name():
    from dvt_amd.dp import FlatParameters
    lin = nn.Linear(3, 2)
    flat = FlatParameters(lin, compute_dtype=None)
    assert "ema" in FlatParameters._STATE_TENSORS and "ema" not in flat.state_dict()
    with pytest.raises(RuntimeError, match="enable_ema first"):
        flat.ema_update()
    ema = flat.enable_ema(0.99)
    assert ema is flat.ema and torch.equal(ema, flat.data) and ema.data_ptr() != flat.data.data_ptr()
    assert float(flat.ema_decay_dev) == pytest.approx(0.99) and flat.ema_decay_dev.dtype == torch.float32
    flat.set_ema_decay(0.5)
    assert float(flat.ema_decay_dev) == 0.5
    flat.ema.mul_(2.0)
    before = flat.data.clone()
    with flat.ema_weights():
        assert torch.equal(lin.weight.detach().reshape(-1), 2.0 * before[:6]) and torch.equal(flat.ema, before)
    assert torch.equal(flat.data, before) and torch.equal(flat.ema, 2.0 * before)
    sd = flat.state_dict()
    other = FlatParameters(nn.Linear(3, 2), compute_dtype=None)
    other.load_state_dict(sd)                                    # an EMA loaded into an object without one enables it
    assert torch.equal(other.ema, flat.ema) and float(other.ema_decay_dev) == 0.5
    flat.set_param_groups([{"params": list(lin.parameters())}])
    flat.scaler = dict(growth_interval=1, growth=2.0, backoff=0.5)       # as enable_loss_scaling leaves it
    with pytest.raises(NotImplementedError, match="adamw_step"):
        flat.adamw_groups_step(1e-3)


# ---------------------------------------------------------------- tests/optim_groups_ref.py
def test_the_interleaved_pattern():
    assert G.interleaved_groups(64 * 9).tolist() == [0, 1, 2, 1, 0, 1, 2, 1, 0]
    assert G.interleaved_groups(65, 2).tolist() == [0, 1] and G.interleaved_groups(5).tolist() == [0]
    blocks, idx = G.group_elements(G.interleaved_groups(257), 1, 257)
    assert blocks.tolist() == [1, 3] and idx.tolist() == list(range(64, 128)) + list(range(192, 256))
    blocks, idx = G.group_elements(G.interleaved_groups(257), 0, 257)
    assert blocks.tolist() == [0, 4] and idx.tolist() == list(range(64)) + [256]


def test_grouped_reference_is_adam_step_per_group_and_torch_adamw():
    n, lr, b1, b2, eps = 64 * 7 + 5, 5e-3, 0.9, 0.999, 1e-8
    gen = torch.Generator().manual_seed(11)
    p, g, m, v = (t.double() for t in O.optim_inputs(n, gen, zero_state=True))
    g64 = G.interleaved_groups(n)
    # per group: optim_ref.adam_step on the group's slice
    got = G.groups_step(p, g, m, v, g64, G.SCALES, G.DECAYS, lr=lr, b1=b1, b2=b2, eps=eps, steps_taken=0)
    for gi in range(3):
        _, idx = G.group_elements(g64, gi, n)
        want = O.adam_step(p[idx], g[idx], m[idx], v[idx], lr=O.f32(O.f32(lr) * O.f32(G.SCALES[gi])), b1=b1, b2=b2, eps=eps,
                           wd=G.DECAYS[gi], steps_taken=0, coupled=False, bias="device")
        assert all(torch.equal(a[idx], b) for a, b in zip(got, want))
    # a skipped block keeps everything
    skip = O.skip_mask(n, [1, -1])
    sk = G.groups_step(p, g, m, v, g64, G.SCALES, G.DECAYS, lr=lr, b1=b1, b2=b2, eps=eps, steps_taken=0, skip=skip)
    mask = skip.bool().repeat_interleave(64)[:n]
    assert all(torch.equal(a[mask], o[mask]) and torch.equal(a[~mask], b[~mask]) for a, o, b in zip(sk, (p, m, v), got))
    # torch.optim.AdamW on the same groups, float64, three steps
    params = []
    for gi in range(3):
        _, idx = G.group_elements(g64, gi, n)
        params.append((idx, nn.Parameter(p[idx].clone())))
    opt = torch.optim.AdamW([{"params": [q], "lr": G.group_lr(lr, G.SCALES[gi]), "weight_decay": O.f32(G.DECAYS[gi])}
                             for gi, (_, q) in enumerate(params)], betas=(O.f32(b1), O.f32(b2)), eps=O.f32(eps))
    state = (p, m, v)
    for t in range(3):
        gt = g * (1.0 + 0.25 * t)
        state = G.groups_step(state[0], gt, state[1], state[2], g64, G.SCALES, G.DECAYS, lr=lr, b1=b1, b2=b2, eps=eps,
                              steps_taken=t)
        for idx, q in params:
            q.grad = gt[idx].clone()
        opt.step()
    for idx, q in params:
        err = (state[0][idx] - q.detach()).abs()
        assert bool((err <= 1e-12 * torch.maximum(q.detach().abs(), torch.tensor(1e-30, dtype=torch.float64))).all())
    assert not torch.equal(state[0], p)


def test_ema_reference_is_timms_formula():
    gen = torch.Generator().manual_seed(5)
    ema, p = torch.randn(300, generator=gen, dtype=torch.float64), torch.randn(300, generator=gen, dtype=torch.float64)
    d = 0.9999
    got = G.ema_step(ema, p, d=d)
    timm = ema.clone()
    timm.copy_(O.f32(d) * timm + (1.0 - O.f32(d)) * p)            # ModelEmaV2: update_fn = lambda e, m: decay * e + (1 - decay) * m
    assert torch.equal(got, timm)
    e32, p32 = torch.tensor([4.0, -2.0, 0.0]), torch.tensor([8.0, 6.0, -1.0])
    assert G.ema_step(e32, p32, d=0.75).tolist() == [5.0, 0.0, -0.25] and G.ema_step(e32, p32, d=0.5).tolist() == [6.0, 2.0, -0.5]
    G.check_ema(G.ema_step(e32, p32, d=0.75), e32, p32, 0.75, "exact")
    with pytest.raises(AssertionError):
        G.check_ema(G.ema_step(e32, p32, d=0.5), e32, p32, 0.75, "wrong decay")
    assert math.isclose(G.group_lr(5e-3, 0.75), 0.00375, rel_tol=1e-6) and G.group_lr(5e-3, 1.0) == O.f32(5e-3)
