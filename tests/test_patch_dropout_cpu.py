"""The float64 reference of patch dropout (tests/patchdrop_ref.py) without a GPU: its rank rule, its gather and the
adjoint, the masked forward and backward against the golden of the imported reference model
(tests/golden/patch_dropout.npz), and -- with every position kept -- against the oracle's full forward."""
import numpy as np
import torch

from oracle import clip_path as O
from tests import patchdrop_ref as R
from tests.util import fill_state_from_numpy, golden, rel_l2


# ---------------------------------------------------------------- the restatement
def test_rank_rule_of_the_restatement():
    keep, slot = R.keep_select(torch.zeros(3, 16, dtype=torch.int32), 5)         # all-equal keys keep 0 .. k-1
    assert keep.dtype == slot.dtype == torch.int32
    assert torch.equal(keep, torch.arange(5, dtype=torch.int32).repeat(3, 1))
    assert torch.equal(slot[:, :5], keep) and bool((slot[:, 5:] == -1).all())
    keys = torch.tensor([[5, 1, 5, 1, 0, 7]], dtype=torch.int32)
    keep, slot = R.keep_select(keys, 3, rows_per=2)                               # order: 4, 1, 3, 0, 2, 5
    assert keep.tolist() == [[1, 3, 4]] * 2 and slot.tolist() == [[-1, 0, -1, 1, 2, -1]] * 2
    assert R.keep_select(keys, 4)[0].tolist() == [[0, 1, 3, 4]]                   # the tie at 5 goes to the lower position
    assert R.keep_select(-keys, 1)[0].tolist() == [[5]]                           # signed order
    g = torch.Generator().manual_seed(1)
    keys = torch.randint(-2 ** 31, 2 ** 31 - 1, (7, 196), generator=g, dtype=torch.int64).to(torch.int32)
    keep, slot = R.keep_select(keys, 98)
    assert bool((keep[:, 1:] > keep[:, :-1]).all()) and torch.equal(R.slots_of(keep, 196), slot)
    kth = torch.sort(keys.long(), dim=1).values[:, 97]
    assert bool((keys.long().gather(1, keep.long()) <= kth[:, None]).all())


def test_restatement_gather_and_its_adjoint():
    from tests import tubelet_ref as TR
    b, t, Cc, H, W, P, pt, k = 2, 4, 3, 32, 32, 8, 2, 5
    x = TR.integer_clip((b, t, Cc, H, W), seed=4)
    keys = torch.from_numpy(np.random.default_rng(5).integers(0, 1000, (b * t // pt, 16))).to(torch.int32)
    keep, slot = R.keep_select(keys, k)
    rows = R.gather_keep(x, P, pt, keep)
    full = TR.gather(x, P, pt).reshape(b * t // pt, 16, -1)
    assert rows.shape == (b * t // pt * k, pt * P * P * Cc)
    for s in range(keep.shape[0]):
        for i in range(k):
            assert torch.equal(rows[s * k + i], full[s, int(keep[s, i])])
    y = TR.integer_clip(tuple(rows.shape), seed=6)
    back = R.scatter_keep(y, x.shape, P, pt, keep)
    assert float((rows * y).sum()) == float((x * back).sum())
    kept_mask = R.scatter_keep(torch.ones_like(rows), x.shape, P, pt, keep)
    assert set(kept_mask.unique().tolist()) == {0.0, 1.0} and float(kept_mask.mean()) == k / 16


def _golden_model():
    from dvt_amd.models.vit import ViViT
    g = golden("patch_dropout.npz")
    cfg = {k[4:]: int(g[k]) for k in g.files if k.startswith("cfg_")}
    net = ViViT(cfg["image"], cfg["patch"], cfg["classes"], cfg["frames"], dim=cfg["dim"], depth=cfg["depth"],
                heads=cfg["heads"], dim_head=cfg["dim_head"])
    fill_state_from_numpy(net.named_parameters(), int(g["fill_seed"]))
    return g, cfg, {k: v.detach().double() for k, v in net.state_dict().items()}


def test_restatement_matches_the_reference_golden():
    g, cfg, P = _golden_model()
    clip, target, keep = (torch.from_numpy(g[k]) for k in ("clip", "target", "keep"))
    assert clip.dtype == torch.float64 and keep.dtype == torch.int32 and keep.shape == (clip.shape[0] * cfg["frames"], 5)
    logits, loss, grads = R.masked_step(clip, target, P, keep, patch=cfg["patch"], depth=cfg["depth"], heads=cfg["heads"])
    errs = {"logits": rel_l2(logits, torch.from_numpy(g["logits"])), "loss": abs(float(loss) - float(g["loss"]))}
    names = [k[2:] for k in g.files if k.startswith("g:")]
    assert sorted(names) == sorted(P)
    for name in names:
        errs[name] = rel_l2(grads[name], torch.from_numpy(g["g:" + name]))
    worst = max(errs, key=errs.get)
    print(f"[patch dropout] restatement against the reference golden: worst {worst} {errs[worst]:.2e}")
    assert all(v <= 1e-9 for v in errs.values()), {k: v for k, v in errs.items() if v > 1e-9}
    # positional rows of positions nobody kept get no gradient, in the reference too
    n = (cfg["image"] // cfg["patch"]) ** 2
    gp = torch.from_numpy(g["g:pos_embedding"])[0]
    kept = R.slots_of(keep, n).reshape(clip.shape[0], cfg["frames"], n).ge(0).any(0)          # [t, n]
    assert bool((gp[:, 1:][~kept] == 0).all()) and bool((gp[:, 1:][kept].abs().sum(-1) > 0).all()) and not bool(kept.all())


def test_restatement_on_tubelets_is_the_per_frame_one_under_central_inflation():
    """pt = 2 with the per-frame weight in the central block: the masked forward of the tubelet model on a clip equals the
    per-frame masked forward on the clip's central frames (the identity tests/test_tubelet_cpu.py proves for the gather)."""
    from dvt_amd.models.vit import inflate_patch_embedding
    g, cfg, P = _golden_model()
    clip, keep = torch.from_numpy(g["clip"]), torch.from_numpy(g["keep"])
    b = clip.shape[0]
    tub = dict(P)
    tub["to_patch_embedding.1.weight"] = inflate_patch_embedding(P["to_patch_embedding.1.weight"], 2, "central")
    tub["pos_embedding"] = P["pos_embedding"][:, 1::2]
    keep2 = keep.reshape(b, cfg["frames"], -1)[:, 1::2].reshape(b * cfg["frames"] // 2, -1).contiguous()
    kw = dict(patch=cfg["patch"], depth=cfg["depth"], heads=cfg["heads"])
    got = R.masked_forward(clip, tub, keep2, pt=2, **kw)
    per_frame = dict(P, pos_embedding=tub["pos_embedding"])
    want = R.masked_forward(clip[:, 1::2], per_frame, keep2, **kw)
    assert rel_l2(got, want) <= 1e-12


def test_restatement_with_every_position_kept_is_the_oracle_forward():
    g, cfg, P = _golden_model()
    clip = torch.from_numpy(g["clip"])
    n = (cfg["image"] // cfg["patch"]) ** 2
    keep = torch.arange(n, dtype=torch.int32).repeat(clip.shape[0] * cfg["frames"], 1)
    got = R.masked_forward(clip, P, keep, patch=cfg["patch"], depth=cfg["depth"], heads=cfg["heads"])
    assert torch.equal(got, O.vivit_forward(clip, P, patch=cfg["patch"], depth=cfg["depth"], heads=cfg["heads"]))
