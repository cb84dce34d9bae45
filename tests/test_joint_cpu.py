"""JointViViT without a GPU: the float64 restatement tests/joint_ref.py against the fixture made from the imported
reference modules (tests/golden/joint_vivit.npz), and the model's surface -- state-dict keys, validation, the layer ids
and the parameter grouping of the fine-tuning recipe."""
import numpy as np
import pytest
import torch

from tests import joint_ref as JR
from tests.util import fill_state_from_numpy, golden


@pytest.fixture(autouse=True, scope="module")
def joint_model_exported():
    """the fixture and the restatement below are the yardsticks of a model the package exports"""
    import dvt_amd.models as M
    assert M.JointViViT is M.joint_vivit.JointViViT


def _model(npz, tag, **kw):
    from dvt_amd.models import JointViViT
    cfg = JR.config(npz)
    pool, pt = JR.VARIANTS[tag]
    net = JointViViT(cfg["image"], cfg["patch"], cfg["classes"], cfg["frames"], dim=cfg["dim"], depth=cfg["depth"],
                     heads=cfg["heads"], pool=pool, dim_head=cfg["dim_head"], tubelet_size=pt, **kw)
    fill_state_from_numpy(net.named_parameters(), int(npz["fill_seed"]))
    return net, cfg, pool, pt


@pytest.mark.parametrize("tag", list(JR.VARIANTS))
def test_joint_ref_reproduces_the_fixture(tag):
    npz = golden("joint_vivit.npz")
    net, cfg, pool, pt = _model(npz, tag)
    assert [n for n, _ in net.named_parameters()] == list(npz[f"{tag}:names"])
    tokens = cfg["frames"] // pt * (cfg["image"] // cfg["patch"]) ** 2 + 1
    assert tokens == (769 if pt == 1 else 385)
    P = {n: p.detach().double() for n, p in net.named_parameters()}
    clip, target = JR.inputs(npz)
    logits, loss, grads = JR.step(clip.double(), P, target.double(), patch=cfg["patch"], depth=cfg["depth"],
                                  heads=cfg["heads"], pool=pool, pt=pt)
    dev = JR.deviations(npz, tag, logits, loss, grads)
    assert set(dev) == {"logits", "loss", "g:clip"} | {"g:" + n for n in P}
    worst = max(dev, key=dev.get)
    assert dev[worst] < 1e-9, (worst, dev[worst])


def test_fixture_holds_the_references_own_deviations():
    npz = golden("joint_vivit.npz")
    for tag in JR.VARIANTS:
        for prec in ("bf16", "fp16"):
            keys = [k for k in npz.files if k.startswith(f"{tag}:dev_{prec}:")]
            assert len(keys) == 2 + len([k for k in npz.files if k.startswith(f"{tag}:gs:")])
            assert all(0 < float(npz[k]) < 0.2 for k in keys)


def test_state_dict_keys_and_shapes():
    from dvt_amd.models import JointViViT
    net = JointViViT(32, 8, 7, 4, dim=64, depth=2, heads=1, dim_head=64, tubelet_size=2)
    sd = net.state_dict()
    want = ["pos_embedding", "cls_token", "to_patch_embedding.1.weight", "to_patch_embedding.1.bias"]
    for i in range(2):
        a, f = f"transformer.layers.{i}.0.", f"transformer.layers.{i}.1."
        want += [a + "norm.weight", a + "norm.bias", a + "fn.to_qkv.weight",
                 f + "norm.weight", f + "norm.bias", f + "fn.net.0.weight", f + "fn.net.0.bias", f + "fn.net.3.weight",
                 f + "fn.net.3.bias"]
    want += ["transformer.norm.weight", "transformer.norm.bias", "mlp_head.0.weight", "mlp_head.0.bias",
             "mlp_head.1.weight", "mlp_head.1.bias"]
    assert list(sd) == want                              # (heads == 1 and dim_head == dim: no output projection, vit.py:34)
    assert tuple(sd["pos_embedding"].shape) == (1, 1, 2 * 16 + 1, 64)
    assert tuple(sd["cls_token"].shape) == (1, 1, 64)
    assert tuple(sd["to_patch_embedding.1.weight"].shape) == (64, 2 * 3 * 8 * 8)
    assert net.num_tokens == 32
    proj = JointViViT(32, 8, 7, 4, dim=64, depth=1, heads=2, dim_head=64)
    assert "transformer.layers.0.0.fn.to_out.0.weight" in proj.state_dict()


def test_validation_errors():
    from dvt_amd.models import JointViViT
    for bad in (0, -1, 1.0, True, "2"):
        with pytest.raises(ValueError, match="tubelet_size"):
            JointViViT(32, 8, 7, 4, tubelet_size=bad)
    with pytest.raises(ValueError, match="multiple of tubelet_size"):
        JointViViT(32, 8, 7, 5, tubelet_size=2)
    with pytest.raises(AssertionError, match="divisible"):
        JointViViT(30, 8, 7, 4)
    with pytest.raises(AssertionError, match="pool"):
        JointViViT(32, 8, 7, 4, pool="max")
    net = JointViViT(32, 8, 7, 4, dim=64, depth=1, heads=1)
    with pytest.raises(ValueError, match=r"\[b, t, c, H, W\]"):
        net(torch.zeros(2, 3, 32, 32))
    with pytest.raises(ValueError, match="5 frames"):
        net(torch.zeros(1, 5, 3, 32, 32))
    with pytest.raises(ValueError, match="16 x 16"):
        net(torch.zeros(1, 4, 3, 16, 16))


def test_layer_ids_cover_every_parameter_and_param_groups_accepts_the_model():
    from dvt_amd import optim
    from dvt_amd.models import JointViViT
    net = JointViViT(32, 8, 7, 4, dim=64, depth=3, heads=2)
    assert net.num_lr_layers == 4
    ids = {name: net.layer_id(name) for name, _ in net.named_parameters()}
    assert ids["pos_embedding"] == ids["cls_token"] == ids["to_patch_embedding.1.weight"] == 0
    assert [ids[f"transformer.layers.{i}.0.fn.to_qkv.weight"] for i in range(3)] == [1, 2, 3]
    assert ids["transformer.norm.weight"] == ids["mlp_head.1.bias"] == 4
    assert set(ids.values()) == set(range(5))
    for bad in ("transformer.layers.3.0.norm.weight", "space_token", "nope"):
        with pytest.raises(KeyError):
            net.layer_id(bad)
    assert net.no_weight_decay() == {"pos_embedding", "cls_token"}
    groups = optim.param_groups(net, 1e-3, 0.05, layer_decay=0.75)
    names = [n for g in groups for n in g["names"]]
    assert sorted(names) == sorted(ids)
    for g in groups:
        layer = {ids[n] for n in g["names"]}
        assert len(layer) == 1
        assert g["lr_scale"] == pytest.approx(0.75 ** (4 - layer.pop()))
        for n in g["names"]:
            p = dict(net.named_parameters())[n]
            decayed = not (p.ndim <= 1 or n.endswith(".bias") or n in net.no_weight_decay())
            assert g["weight_decay"] == (0.05 if decayed else 0.0)
    plain = optim.param_groups(net, 1e-3, 0.05)
    assert len(plain) == 2 and sum(len(g["params"]) for g in plain) == len(ids)


def test_digest_rule_is_the_shared_one():
    """the positional table's digest carries its CLS row (tests.util.digest_idx), the clip's the 256 spaced entries"""
    npz = golden("joint_vivit.npz")
    assert npz["cls_t1:gs:pos_embedding"].size == 128 + 256 and npz["cls_t1:gs:clip"].size == 256
    assert np.isfinite(npz["cls_t1:logits"]).all()
