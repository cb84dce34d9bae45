"""The float64 reference of stochastic depth (tests/droppath_ref.py) without a GPU: against the golden of the imported
reference model run on ``x[keep]`` (tests/golden/drop_path.npz), its gather / scatter pair as adjoints, and -- with nothing
dropped -- against the oracle's full forward."""
import numpy as np
import pytest
import torch

from oracle import clip_path as O
from tests import droppath_ref as R
from tests.util import fill_state_from_numpy, golden, rel_l2


def _golden_model():
    from dvt_amd.models.vit import ViViT
    g = golden("drop_path.npz")
    cfg = {k[4:]: int(g[k]) for k in g.files if k.startswith("cfg_")}
    net = ViViT(cfg["image"], cfg["patch"], cfg["classes"], cfg["frames"], dim=cfg["dim"], depth=cfg["depth"],
                heads=cfg["heads"], dim_head=cfg["dim_head"])
    fill_state_from_numpy(net.named_parameters(), int(g["fill_seed"]))
    return g, {k: v.detach().double() for k, v in net.state_dict().items()}


def test_the_fixture_has_the_geometry_and_the_keep_sets_it_is_meant_to():
    g = golden("drop_path.npz")
    cfg, clip, target, keeps, patch_keep = R.fixture(g)
    assert (cfg["image"], cfg["patch"], cfg["frames"], cfg["depth"], cfg["dim"], cfg["heads"]) == (32, 8, 4, 2, 32, 2)
    assert clip.shape == (3, 4, 3, 32, 32) and len(keeps) == 4 * cfg["depth"] and patch_keep.shape == (12, 5)
    S = [12] * 4 + [3] * 4
    assert any(e is None for e in keeps)
    assert any(e is not None and e.numel() == 1 for e in keeps)
    assert any(e is not None and e.numel() == s for e, s in zip(keeps, S))
    for e, s in zip(keeps, S):
        if e is not None:
            assert e.dtype == torch.int32 and bool((e[1:] > e[:-1]).all()) and 0 <= int(e[0]) and int(e[-1]) < s


@pytest.mark.parametrize("case", sorted(R.CASES))
def test_restatement_matches_the_reference_golden(case):
    g, P = _golden_model()
    cfg, clip, target, keeps, patch_keep = R.fixture(g)
    mode, with_patches = R.CASES[case]
    scales = R.alphas(keeps, 12, 3, cfg["depth"], float(g["drop_path"]), mode)
    logits, loss, grads = R.step(clip, target, P, keeps, scales, patch=cfg["patch"], depth=cfg["depth"], heads=cfg["heads"],
                                 patch_keep=patch_keep if with_patches else None)
    errs = R.digest_errors(g, case, logits, grads)
    assert len(errs) == len(P) + 1
    worst = max(errs, key=errs.get)
    assert errs[worst] <= 1e-9, (worst, errs[worst])
    assert abs(float(loss) - float(g[f"{case}:loss"])) <= 1e-12


def test_the_scales_follow_the_mode():
    keeps = [torch.arange(7, dtype=torch.int32), None, torch.arange(1, dtype=torch.int32), None,
             torch.arange(2, dtype=torch.int32), None, None, torch.arange(3, dtype=torch.int32)]
    assert R.alphas(keeps, 12, 3, 2, 0.3, "subset") == [12 / 7, None, 12.0, None, 1.5, None, None, 1.0]
    r = R.rates(2, 0.3)
    assert r == pytest.approx([0.0, 0.1, 0.2, 0.3])
    assert R.alphas(keeps, 12, 3, 2, 0.3, "bernoulli") == [1.0, None, 1 / (1 - r[1]), None, 1 / (1 - r[2]), None, None,
                                                           1 / (1 - r[3])]
    assert R.kept(256, 0.1) == 231 and R.kept(8, 0.1) == 8 and R.kept(8, 0.125) == 7 and R.kept(12, 0.5) == 6


def test_nothing_dropped_is_the_oracle_forward():
    g, P = _golden_model()
    cfg, clip, target, keeps, _ = R.fixture(g)
    full = [torch.arange(12, dtype=torch.int32)] * 4 + [torch.arange(3, dtype=torch.int32)] * 4
    for dk in ([None] * 8, full):
        scales = R.alphas(dk, 12, 3, cfg["depth"], 0.3, "subset")
        got = R.forward(clip, P, dk, scales, patch=cfg["patch"], depth=cfg["depth"], heads=cfg["heads"])
        want = O.vivit_forward(clip, P, patch=cfg["patch"], depth=cfg["depth"], heads=cfg["heads"])
        assert rel_l2(got, want) <= 1e-14


def test_gather_and_scatter_add_are_adjoints():
    rng = np.random.default_rng(11)
    S, k, shape = 9, 4, (5, 6)
    x = torch.from_numpy(rng.standard_normal((S,) + shape))
    y = torch.from_numpy(rng.standard_normal((k,) + shape))
    keep = torch.from_numpy(np.sort(rng.permutation(S)[:k]).astype(np.int32))
    slot = R.slots_of(keep, S)
    assert slot.dtype == torch.int32 and slot[keep.long()].tolist() == list(range(k)) and int((slot < 0).sum()) == S - k
    alpha = 12 / 11
    lhs = float((R.gather(x, keep, alpha) * y).sum())
    rhs = float((x * R.scatter_add(torch.zeros_like(x), y, slot, alpha)).sum())
    assert lhs == pytest.approx(rhs, rel=1e-14)
    # exact on integers with a power-of-two scale, a dropped index included
    xi = torch.from_numpy(rng.integers(-8, 9, (S,) + shape).astype(np.float64))
    yi = torch.from_numpy(rng.integers(-8, 9, (k,) + shape).astype(np.float64))
    idx = keep.clone()
    idx[1] = -1
    sl = R.slots_of(keep, S)
    sl[int(keep[1])] = -1
    assert float((R.gather(xi, idx, 0.5) * yi).sum()) == float((xi * R.scatter_add(torch.zeros_like(xi), yi, sl, 0.5)).sum())
    assert bool((R.gather(xi, idx, 2.0)[1] == 0).all())
    # the rule as the model uses it: res + alpha * y in the kept rows, res elsewhere
    out = R.scatter_add(xi, yi, slot, 2.0)
    for s in range(S):
        want = xi[s] + 2.0 * yi[int(slot[s])] if int(slot[s]) >= 0 else xi[s]
        assert torch.equal(out[s], want)
    # 16-bit gather: the fp32 product rounded once
    xb = x.to(torch.bfloat16)
    assert torch.equal(R.gather(xb, keep, alpha), (xb[keep.long()].float() * torch.tensor(alpha, dtype=torch.float32)).to(torch.bfloat16))
