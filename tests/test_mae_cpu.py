"""Masked-autoencoder pre-training without a GPU: the float64 statement tests/mae_ref.py against the golden of the imported
reference modules (tests/golden/mae.npz, tools/gen_golden_mae.py), the adjoint identity of the restore, and the host surface
of ``MaskedClipAutoencoder``, the header and the built library."""
from __future__ import annotations

import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

from tests import mae_ref as M
from tests import patchdrop_ref as PR
from tests.util import fill_state_from_numpy, golden, rel_l2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY_POINTS = ("dvt_tokens_restore_fwd", "dvt_tokens_restore_bwd", "dvt_mae_loss_fwd", "dvt_mae_loss_bwd")
CFG = dict(dim=32, depth=1, heads=2, dim_head=16)
DEC = dict(decoder_dim=32, decoder_depth=1, decoder_heads=2, decoder_dim_head=16)
UNTRAINED = ("encoder.temporal_transformer.", "encoder.temporal_token", "encoder.mlp_head.")


@functools.lru_cache(maxsize=None)
def _golden():
    g = golden("mae.npz")
    return g, {k[4:]: int(g[k]) for k in g.files if k.startswith("cfg_")}


def _golden_net(**kw):
    from dvt_amd.models.mae import MaskedClipAutoencoder
    from dvt_amd.models.vit import ViViT
    g, cfg = _golden()
    enc = ViViT(cfg["image"], cfg["patch"], cfg["classes"], cfg["frames"], dim=cfg["dim"], depth=cfg["depth"],
                heads=cfg["heads"], dim_head=cfg["dim_head"], compute_dtype=torch.float32)
    net = MaskedClipAutoencoder(enc, decoder_dim=cfg["dec_dim"], decoder_depth=cfg["dec_depth"], decoder_heads=cfg["dec_heads"],
                                decoder_dim_head=cfg["dec_dim_head"], mask_ratio=0.7, **kw)
    fill_state_from_numpy(net.named_parameters(), int(g["fill_seed"]))
    return net


@pytest.mark.parametrize("tag", ["norm", "raw"])
def test_the_restatement_against_the_reference_golden(tag):
    g, cfg = _golden()
    net = _golden_net()
    assert [name for name, _ in net.named_parameters()] == list(g["names"])       # one fill serves both sides
    P = {k: v.detach().double() for k, v in net.state_dict().items()}
    clip, keep = torch.from_numpy(g["clip"]).double(), torch.from_numpy(g["keep"])
    loss, per, grads = M.masked_step(clip, P, keep, patch=cfg["patch"], depth=cfg["depth"], heads=cfg["heads"],
                                     dec_depth=cfg["dec_depth"], dec_heads=cfg["dec_heads"], norm_pix=tag == "norm")
    stored = {k[len(tag) + 3:]: torch.from_numpy(g[k]) for k in g.files if k.startswith(tag + ":g:")}
    assert sorted(stored) == sorted(grads) and len(stored) > 20
    assert not any(name.startswith(UNTRAINED) for name in stored)
    assert all(name in stored or name.startswith(UNTRAINED) for name in P)
    errs = {"loss": abs(float(loss) - float(g[tag + ":loss"])) / abs(float(g[tag + ":loss"])),
            "per_patch": rel_l2(per, torch.from_numpy(g[tag + ":per_patch"]))}
    errs.update({name: rel_l2(grads[name], ref) for name, ref in stored.items()})
    assert all(v <= 1e-9 for v in errs.values()), {k: v for k, v in errs.items() if v > 1e-9}
    # kept positions carry no loss, and the closed-form gradient of the loss is autograd's
    slot = PR.slots_of(keep, 16)
    assert bool((per[slot >= 0] == 0).all()) and bool((per[slot < 0] > 0).all())
    pred = torch.randn(8, 16, 192, dtype=torch.float64, generator=torch.Generator().manual_seed(3)).requires_grad_()
    ls, _ = M.loss(pred, clip, slot, cfg["patch"], 1, tag == "norm")
    (auto,) = torch.autograd.grad(ls * 3.0, pred)
    assert rel_l2(M.loss_grad(pred.detach(), clip, slot, cfg["patch"], 1, tag == "norm", g=3.0), auto) <= 1e-12


def test_the_golden_tells_the_two_losses_and_the_variance_rule_apart():
    g, cfg = _golden()
    assert abs(float(g["norm:loss"]) - float(g["raw:loss"])) > 1e-3
    clip = torch.from_numpy(g["clip"]).double()
    t = M.targets(clip, cfg["patch"], 1, True)
    D = t.shape[-1]
    # unbiased variance: a normalised patch has sum of squares (D - 1) var / (var + eps), just under D - 1 -- not D
    ss = (t ** 2).sum(-1)
    assert bool((ss < D - 1).all()) and bool((ss > D - 1 - 1e-3).all())


@pytest.mark.parametrize("shape", [(8, 4, 16, 5, 32, 1), (4, 2, 9, 9, 8, 0), (6, 3, 10, 1, 16, 2)],
                         ids=lambda s: "x".join(map(str, s)))
def test_restore_adjoint_identity(shape):
    """<restore(y, mask, pos), g> = <y, dy> + <mask, dmask> + <pos, dpos> in float64, and the adjoint is autograd's."""
    S, T, n, k, d, skip = shape
    gen = torch.Generator().manual_seed(sum(shape))
    y, mask, pos, g = (torch.randn(*s, dtype=torch.float64, generator=gen)
                       for s in ((S, skip + k, d), (d,), (T, n, d), (S, n, d)))
    keys = torch.randint(0, 1000, (S, n), generator=gen).to(torch.int32)
    keep, slot = PR.keep_select(keys, k)
    out = M.restore(y, mask, pos, slot, skip)
    for s in range(S):
        for j in range(n):
            src = y[s, skip + int(slot[s, j])] if slot[s, j] >= 0 else mask
            assert torch.equal(out[s, j], src + pos[s % T, j])
    dy, dmask, dpos = M.restore_adjoint(g, keep, slot, T, skip)
    lhs = float((out * g).sum())
    rhs = float((y * dy).sum() + (mask * dmask).sum() + (pos * dpos).sum())
    assert abs(lhs - rhs) <= 1e-12 * max(1.0, abs(lhs))
    assert bool((dy[:, :skip] == 0).all())
    if k == n:
        assert bool((dmask == 0).all())
    leaves = [v.clone().requires_grad_() for v in (y, mask, pos)]
    M.restore(*leaves, slot, skip).backward(g)
    assert all(rel_l2(a, b.grad) <= 1e-14 for a, b in zip((dy, dmask, dpos), leaves))


def test_constructor_arguments_and_errors():
    from dvt_amd.models import MaskedClipAutoencoder
    from dvt_amd.models.vit import ViViT
    params = inspect.signature(MaskedClipAutoencoder.__init__).parameters
    defaults = dict(decoder_dim=384, decoder_depth=4, decoder_heads=6, decoder_dim_head=64, decoder_scale_dim=4, mask_ratio=0.9,
                    mask_mode="tube", norm_pix_loss=True)
    assert list(params) == ["self", "encoder"] + list(defaults)
    for name, default in defaults.items():
        assert params[name].kind is inspect.Parameter.KEYWORD_ONLY and params[name].default == default
    assert list(inspect.signature(MaskedClipAutoencoder.forward).parameters) == ["self", "x", "keep"]

    def make(ratio=0.9, mode="tube", image=32):
        return MaskedClipAutoencoder(ViViT(image, 8, 19, 4, **CFG), mask_ratio=ratio, mask_mode=mode, **DEC)

    # n = 16: k = 16 - floor(ratio * 16)
    assert make(0.9).num_kept(16) == 2 and make(0.7).num_kept(16) == 5 and make(0.99).num_kept(16) == 1
    assert make(0.9).num_kept(196) == 20 and make(0.75).num_kept(196) == 49
    for ratio in (0.0, 0.05, 1.0, -0.1, 1.5):                      # k == n, k == n, k < 1, out of range twice
        with pytest.raises(ValueError, match="mask_ratio"):
            make(ratio)
    with pytest.raises(ValueError, match="mask_ratio"):
        make(0.9, image=8)                                          # n = 1 cannot be masked
    with pytest.raises(ValueError, match="mask_mode"):
        make(mode="block")
    with pytest.raises(TypeError, match="ViViT"):
        MaskedClipAutoencoder(torch.nn.Linear(2, 2))
    with pytest.raises(ValueError, match="decoder_dim"):
        MaskedClipAutoencoder(ViViT(32, 8, 19, 4, **CFG), decoder_dim=36, decoder_depth=1, decoder_heads=2, decoder_dim_head=16)


def test_state_dict_keys_and_the_encoder_round_trip():
    from dvt_amd.models.vit import ViViT
    net = _golden_net()
    sd = net.state_dict()
    enc_keys = ["encoder." + k for k in ViViT(32, 8, 19, 4, **CFG).state_dict()]
    dec_keys = ["decoder." + k[len("space_transformer."):] for k in ViViT(32, 8, 19, 4, **CFG).state_dict()
                if k.startswith("space_transformer.")]
    own = ["mask_token", "decoder_pos_embedding", "decoder_embed.weight", "decoder_embed.bias", "decoder_pred.weight",
           "decoder_pred.bias"]
    assert sorted(sd) == sorted(enc_keys + dec_keys + own)
    assert sd["mask_token"].shape == (1, 1, 32) and sd["decoder_pos_embedding"].shape == (1, 4, 16, 32)
    assert sd["decoder_embed.weight"].shape == (32, 32) and sd["decoder_pred.weight"].shape == (192, 32)
    assert "decoder.norm.weight" in sd                                  # the final norm is part of the decoder
    fresh = ViViT(32, 8, 19, 4, compute_dtype=torch.float32, **CFG)
    result = fresh.load_state_dict(net.encoder_state_dict(), strict=True)
    assert not result.missing_keys and not result.unexpected_keys
    assert all(torch.equal(v, net.encoder.state_dict()[k]) for k, v in fresh.state_dict().items())
    # a tubelet encoder: one temporal token per pt frames, targets of pt * P * P * C values
    from dvt_amd.models import MaskedClipAutoencoder
    tub = MaskedClipAutoencoder(ViViT(32, 8, 19, 4, tubelet_size=2, **CFG), mask_ratio=0.7, **DEC)
    assert tub.decoder_pos_embedding.shape == (1, 2, 16, 32) and tub.decoder_pred.weight.shape == (384, 32)


def test_a_bad_keep_is_refused_on_the_host_and_there_is_no_cpu_path():
    net = _golden_net()
    x = torch.zeros(2, 4, 3, 32, 32)
    good = torch.arange(5, dtype=torch.int32).repeat(8, 1)
    for keep in (good.long(), good[:7], good[0], torch.zeros(8, 0, dtype=torch.int32),
                 torch.arange(16, dtype=torch.int32).repeat(8, 1), torch.arange(17, dtype=torch.int32).repeat(8, 1)):
        with pytest.raises(ValueError, match="keep"):
            net(x, keep=keep)
    with pytest.raises(ValueError, match="keep is on"):
        net(x, keep=good.to("meta"))
    for mode in (net.train, net.eval):
        mode()
        with pytest.raises(RuntimeError, match="no CPU path"):
            net(x, keep=good)
        with pytest.raises(RuntimeError, match="no CPU path"):
            net(x)
    assert "oracle" not in open(os.path.join(ROOT, "data-efficient-video-transformers_amd", "models", "mae.py")).read()


def test_header_declares_and_library_exports_the_entry_points():
    from dvt_amd import _lib
    code = re.sub(r"/\*.*?\*/", " ", open(os.path.join(ROOT, "include", "dvt_hip.h")).read(), flags=re.S)
    lib = _lib.load()
    for name in ENTRY_POINTS:
        (params,) = re.findall(rf"\bint\s+{name}\s*\(([^()]*)\)\s*;", code)
        res, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == params.count(",") + 1 and None not in argtypes, name
        assert "dvt_stream_t stream" in params.split(",")[-1], name
        assert hasattr(lib, name), name
    assert _lib.ABI_VERSION == 5 and lib.dvt_version() == 5
    assert os.path.exists(os.path.join(os.path.dirname(_lib.LIB_PATH), "csrc", "mae.hip"))


def test_launchers_refuse_bad_arguments_before_any_launch():
    from dvt_amd import _lib
    lib = _lib.load()
    one = 16                                   # any non-null, 16-byte aligned address: refused before it is used
    f32 = _lib.F32
    # restore: (y, mask, pos, slot, out, S, T, n, k, skip, d, dtype, stream)
    assert lib.dvt_tokens_restore_fwd(one, one, one, one, one, 4, 2, 16, 5, 1, 36, f32, None) == -1            # d % 8
    assert b"dvt_tokens_restore_fwd" in lib.dvt_last_error() and b"multiple of 8" in lib.dvt_last_error()
    for S, T, n, k, skip, d in ((4, 3, 16, 5, 1, 32), (4, 2, 16, 17, 1, 32), (4, 2, 16, 0, 1, 32), (4, 2, 16, 5, -1, 32)):
        assert lib.dvt_tokens_restore_fwd(one, one, one, one, one, S, T, n, k, skip, d, f32, None) == -1, (S, T, n, k, skip, d)
        assert lib.dvt_tokens_restore_bwd(one, one, one, one, one, one, one, S, T, n, k, skip, d, f32, 0, None) == -1
    assert lib.dvt_tokens_restore_fwd(one, None, one, one, one, 4, 2, 16, 5, 1, 32, f32, None) == -1
    assert lib.dvt_tokens_restore_bwd(one, one, one, one, one, one, one, 4, 2, 16, 5, 1, 36, f32, 0, None) == -1
    assert lib.dvt_tokens_restore_bwd(one, one, one, one, one, one, None, 4, 2, 16, 5, 1, 32, f32, 0, None) == -1
    # loss: (pred, pdt, clip, cdt, slot, per_patch, stats, loss, frames, C, H, W, P, pt, k, norm_pix, eps, stream)
    ok = (8, 3, 32, 32, 8, 2)
    assert lib.dvt_mae_loss_fwd(one, f32, one, f32, one, one, one, one, *ok, 16, 1, 1e-6, None) == -1          # k == n: M == 0
    assert b"M == 0" in lib.dvt_last_error()
    assert lib.dvt_mae_loss_fwd(one, f32, one, f32, one, one, one, one, *ok, 0, 1, 1e-6, None) == -1
    assert lib.dvt_mae_loss_fwd(one, f32, one, f32, one, one, one, one, 7, 3, 32, 32, 8, 2, 5, 1, 1e-6, None) == -1   # 7 frames
    assert lib.dvt_mae_loss_fwd(one, f32, one, f32, one, one, one, one, 8, 3, 32, 36, 8, 2, 5, 1, 1e-6, None) == -1   # W % P
    assert lib.dvt_mae_loss_fwd(one, f32, one, f32, one, one, None, one, *ok, 5, 1, 1e-6, None) == -1          # norm_pix, no stats
    assert lib.dvt_mae_loss_fwd(one, f32, one, f32, one, one, one, one, 1, 3, 8, 8, 8, 1, 1, 1, 1e-6, None) == -1     # n = 1
    assert lib.dvt_mae_loss_bwd(one, f32, one, f32, one, one, one, one, *ok, 16, 1, None) == -1
    assert lib.dvt_mae_loss_bwd(one, f32, one, f32, one, one, None, one, *ok, 5, 1, None) == -1                # no gloss
    assert b"dvt_mae_loss_bwd" in lib.dvt_last_error()


def test_ops_and_functional_signatures_and_host_checks():
    from dvt_amd import functional as F
    from dvt_amd import ops
    assert list(inspect.signature(F.tokens_restore).parameters) == ["y", "mask_token", "pos", "keep", "slot", "S", "T", "skip"]
    assert inspect.signature(F.tokens_restore).parameters["skip"].default == 1
    assert list(inspect.signature(F.mae_loss).parameters) == ["pred", "clip", "slot", "k", "patch", "tubelet", "norm_pix"]
    assert inspect.signature(F.mae_loss).parameters["norm_pix"].default is True
    for name in ("tokens_restore_fwd", "tokens_restore_bwd", "mae_loss_fwd", "mae_loss_bwd"):
        assert callable(getattr(ops, name))
    slot = torch.zeros(4, 16, dtype=torch.int32)
    with pytest.raises(ValueError, match="multiple of 8"):
        ops.tokens_restore_fwd(torch.zeros(4, 6, 36), torch.zeros(36), torch.zeros(2, 16, 36), slot, 5)
    with pytest.raises(ValueError, match="int32"):
        ops.tokens_restore_fwd(torch.zeros(4, 6, 32), torch.zeros(32), torch.zeros(2, 16, 32), slot.long(), 5)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.tokens_restore_fwd(torch.zeros(4, 6, 32), torch.zeros(32), torch.zeros(2, 16, 32), slot, 5)
    with pytest.raises(ValueError, match="M == 0"):
        ops.mae_loss_fwd(torch.zeros(1, 1, 192), torch.zeros(1, 1, 3, 8, 8), torch.zeros(1, 1, dtype=torch.int32), 1, 8, 1, True)
    with pytest.raises(ValueError, match="pred"):
        ops.mae_loss_fwd(torch.zeros(4, 16, 100), torch.zeros(1, 4, 3, 32, 32), slot, 5, 8, 1, True)
    assert ops.MAE_EPS == 1e-6 == M.EPS
