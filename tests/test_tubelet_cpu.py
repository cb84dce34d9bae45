"""Tubelet embedding without a GPU: the two formulations of tests/tubelet_ref.py against each other, the inflation
identities, the model surface, ``ViViT.load_frame_checkpoint`` and the argument checks of the two C entry points."""
import inspect

import pytest
import torch

from oracle import clip_path as O
from tests import tubelet_ref as R

CFG = dict(dim=64, depth=2, heads=2, dim_head=32)


# ---------------------------------------------------------------- the restatement itself
@pytest.mark.parametrize("shape", R.GATHER_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_the_two_formulations_agree_exactly(shape):
    b, t, C, H, W, P, pt = shape
    x = R.integer_clip((b, t, C, H, W), seed=sum(shape))
    a, c = R.gather(x, P, pt), R.gather_conv3d(x, P, pt)
    assert a.dtype == torch.float64 and a.shape == (b * (t // pt) * (H // P) * (W // P), pt * P * P * C)
    assert torch.equal(a, c)
    nh, nw = H // P, W // P
    # the matrix the wrapper allocates for this clip is the restatement's
    from dvt_amd import ops
    frames, *chw = ops._tubelet_geometry(x.shape, P, pt, "tubelet_patchify")
    assert (frames, *chw) == (b * t, C, H, W) and (frames // pt * nh * nw, pt * P * P * C) == a.shape
    if pt >= 2:                                # pt + 1 frames are whole tubelets at pt = 1: nothing to refuse there
        with pytest.raises(ValueError, match="tubelets"):
            ops._tubelet_geometry((b, pt + 1, C, H, W), P, pt, "tubelet_patchify")
    # the definition, entry by entry, on a few hundred random entries
    g = torch.Generator().manual_seed(5)
    for _ in range(300):
        bi, tau, ph, pw = (int(torch.randint(n, (1,), generator=g)) for n in (b, t // pt, nh, nw))
        k, p1, p2, ch = (int(torch.randint(n, (1,), generator=g)) for n in (pt, P, P, C))
        assert a[((bi * (t // pt) + tau) * nh + ph) * nw + pw, ((k * P + p1) * P + p2) * C + ch] == \
            x[bi, tau * pt + k, ch, ph * P + p1, pw * P + p2]
    # a row is the pt per-frame patch vectors of the reference order, concatenated
    pf = R.per_frame_gather(x, P).reshape(b, t // pt, pt, nh * nw, P * P * C)
    assert torch.equal(a.reshape(b, t // pt, nh * nw, pt, P * P * C), pf.permute(0, 1, 3, 2, 4))
    # pt = 1 is the per-frame restatement (and the oracle's)
    one = R.gather(x, P, 1)
    assert torch.equal(one, R.per_frame_gather(x, P)) and torch.equal(one, O.patchify(x, P).reshape(one.shape))
    assert torch.equal(R.gather_conv3d(x, P, 1), one)


INFLATE_SHAPES = [s for s in R.GATHER_SHAPES if s[-1] in (2, 4)]


@pytest.mark.parametrize("shape", INFLATE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_inflation_identities_are_exact(shape):
    from dvt_amd.models.vit import inflate_patch_embedding
    b, t, C, H, W, P, pt = shape
    d, pd = 5, P * P * C
    x = R.integer_clip((b, t, C, H, W), seed=11 + sum(shape))
    w2d = R.integer_clip((d, pd), seed=12, lo=-4, hi=5)
    bias = R.integer_clip((d,), seed=13)
    # central: the tubelet embedding of x is the per-frame embedding of x[:, pt//2::pt]
    wc = inflate_patch_embedding(w2d, pt, "central")
    assert wc.shape == (d, pt * pd) and wc.dtype == torch.float64
    blocks = wc.reshape(d, pt, pd)
    assert torch.equal(blocks[:, pt // 2], w2d) and float(blocks.abs().sum()) == float(w2d.abs().sum())
    want = R.per_frame_embed(x[:, pt // 2::pt], w2d, bias, P)
    assert torch.equal(R.embed_conv3d(x, wc, bias, P, pt), want)
    assert torch.equal(R.gather(x, P, pt) @ wc.t() + bias, want)
    # average: on a clip whose frames repeat within each tubelet, the per-frame embedding of the un-repeated clip
    wa = inflate_patch_embedding(w2d, pt, "average")
    assert torch.equal(wa.reshape(d, pt, pd), (w2d / pt)[:, None].expand(d, pt, pd))
    base = x[:, :t // pt]
    rep = base.repeat_interleave(pt, dim=1)
    want = R.per_frame_embed(base, w2d, bias, P)
    assert torch.equal(R.embed_conv3d(rep, wa, bias, P, pt), want)
    assert torch.equal(R.gather(rep, P, pt) @ wa.t() + bias, want)


def test_inflate_refuses_bad_arguments():
    from dvt_amd.models.vit import inflate_patch_embedding
    w = torch.zeros(4, 12)
    assert torch.equal(inflate_patch_embedding(w + 1, 1, "central"), w + 1)
    assert torch.equal(inflate_patch_embedding(w + 1, 1, "average"), w + 1)
    with pytest.raises(ValueError, match="mode"):
        inflate_patch_embedding(w, 2, "first")
    with pytest.raises(ValueError, match="tubelet_size"):
        inflate_patch_embedding(w, 0, "central")
    with pytest.raises(ValueError, match="weight"):
        inflate_patch_embedding(torch.zeros(4), 2, "central")


# ---------------------------------------------------------------- the model surface
def test_vivit_tubelet_surface():
    from dvt_amd.models.vit import ViViT, Patchify
    net = ViViT(32, 8, 19, 4, tubelet_size=2, **CFG)
    one = ViViT(32, 8, 19, 4, **CFG)
    assert net.tubelet_size == 2 and one.tubelet_size == 1 and net.num_frames == 4
    assert net.to_patch_embedding[1].weight.shape == (64, 2 * 8 * 8 * 3)
    assert net.pos_embedding.shape == (1, 2, 17, 64)
    assert one.to_patch_embedding[1].weight.shape == (64, 8 * 8 * 3) and one.pos_embedding.shape == (1, 4, 17, 64)
    assert list(net.state_dict()) == list(one.state_dict())
    other = {k for k in net.state_dict() if k not in ("to_patch_embedding.1.weight", "pos_embedding")}
    assert all(net.state_dict()[k].shape == one.state_dict()[k].shape for k in other)
    # keyword-only and last
    params = list(inspect.signature(ViViT.__init__).parameters.values())
    assert params[-1].name == "tubelet_size" and params[-1].kind is inspect.Parameter.KEYWORD_ONLY and params[-1].default == 1
    with pytest.raises(ValueError, match="tubelet_size"):
        ViViT(32, 8, 19, 5, tubelet_size=2, **CFG)
    with pytest.raises(ValueError, match="tubelet_size"):
        ViViT(32, 8, 19, 4, tubelet_size=0, **CFG)
    # num_frames stays the number of pixel frames of a clip
    with pytest.raises(ValueError, match="frames"):
        net(torch.zeros(1, 2, 3, 32, 32))
    with pytest.raises(RuntimeError, match="no CPU path"):
        net(torch.randn(1, 4, 3, 32, 32))
    p = Patchify(8, tubelet_size=2)
    assert p.patch_size == 8 and p.tubelet_size == 2 and Patchify(8).tubelet_size == 1
    with pytest.raises(RuntimeError, match="no CPU path"):
        p(torch.randn(1, 4, 3, 32, 32))


def test_ops_and_functional_need_the_gpu_and_check_their_arguments():
    from dvt_amd import functional as F
    from dvt_amd import ops
    x = torch.zeros(1, 4, 3, 16, 16)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.tubelet_patchify(x, 8, 2, torch.float32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        ops.tubelet_patchify_bwd(torch.zeros(4, 768), x.shape, 8, 2, torch.float32)
    with pytest.raises(RuntimeError, match="no CPU path"):
        F.patch_embed(x, torch.zeros(8, 384), torch.zeros(8), 8, torch.float32, tubelet=2)
    assert list(inspect.signature(F.patch_embed).parameters) == ["clip", "w", "b", "patch", "dtype", "tubelet"]
    assert inspect.signature(F.patch_embed).parameters["tubelet"].default == 1


# ---------------------------------------------------------------- checkpoint inflation
@pytest.mark.parametrize("mode", ["central", "average"])
def test_load_frame_checkpoint_block_by_block(mode):
    from dvt_amd.models.vit import ViViT
    torch.manual_seed(3)
    src = ViViT(32, 8, 19, 4, **CFG)
    net = ViViT(32, 8, 19, 4, tubelet_size=2, **CFG)
    sd = {k: v.clone() for k, v in src.state_dict().items()}
    net.load_frame_checkpoint(sd, mode=mode)
    got = net.state_dict()
    w2d, pos = sd["to_patch_embedding.1.weight"], sd["pos_embedding"]
    blocks = got["to_patch_embedding.1.weight"].reshape(64, 2, 192)
    if mode == "central":
        assert torch.equal(blocks[:, 1], w2d) and not blocks[:, 0].any()
        assert torch.equal(got["pos_embedding"], pos[:, 1::2])
    else:
        assert torch.equal(blocks[:, 0], w2d / 2) and torch.equal(blocks[:, 1], w2d / 2)
        assert torch.equal(got["pos_embedding"], (pos[:, 0::2] + pos[:, 1::2]) / 2)
    for k, v in sd.items():
        if k not in ("to_patch_embedding.1.weight", "pos_embedding"):
            assert torch.equal(got[k], v), k
    assert all(torch.equal(v, src.state_dict()[k]) for k, v in sd.items())          # the checkpoint is not written to


def test_load_frame_checkpoint_names_the_mismatched_key():
    from dvt_amd.models.vit import ViViT
    src = ViViT(32, 8, 19, 4, **CFG)
    net = ViViT(32, 8, 19, 4, tubelet_size=2, **CFG)
    before = {k: v.clone() for k, v in net.state_dict().items()}
    sd = dict(src.state_dict())
    missing = {k: v for k, v in sd.items() if k != "space_token"}
    with pytest.raises(ValueError, match="space_token"):
        net.load_frame_checkpoint(missing)
    with pytest.raises(ValueError, match="extra.weight"):
        net.load_frame_checkpoint(dict(sd, **{"extra.weight": torch.zeros(1)}))
    with pytest.raises(ValueError, match=r"mlp_head\.1\.bias"):
        net.load_frame_checkpoint(dict(sd, **{"mlp_head.1.bias": torch.zeros(20)}))
    # a checkpoint of another num_frames, and one that already is a tubelet model's
    with pytest.raises(ValueError, match="pos_embedding"):
        net.load_frame_checkpoint(ViViT(32, 8, 19, 2, **CFG).state_dict())
    with pytest.raises(ValueError, match="pos_embedding"):
        net.load_frame_checkpoint(ViViT(32, 8, 19, 4, tubelet_size=2, **CFG).state_dict())
    with pytest.raises(ValueError, match=r"to_patch_embedding\.1\.weight"):
        net.load_frame_checkpoint(dict(sd, **{"to_patch_embedding.1.weight": torch.zeros(64, 384)}))
    with pytest.raises(ValueError, match="mode"):
        net.load_frame_checkpoint(sd, mode="first")
    assert all(torch.equal(v, before[k]) for k, v in net.state_dict().items())      # nothing was written by a refused load


# ---------------------------------------------------------------- the C ABI without a device
def test_null_and_bad_arguments_fail_before_any_hip_call():
    from dvt_amd import _lib
    lib = _lib.load()
    for name in ("dvt_tubelet_patchify", "dvt_tubelet_patchify_bwd"):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 11
        fn = getattr(lib, name)
        assert fn(None, 0, None, 0, 4, 3, 16, 16, 8, 2, None) == -1 and name.encode() in lib.dvt_last_error()
        # non-null pointers from here on: the checks below fire before either is touched
        assert fn(256, 0, 256, 0, 3, 3, 16, 16, 8, 2, None) == -1                  # frames = 3, pt = 2
        assert name.encode() in lib.dvt_last_error() and b"tubelet" in lib.dvt_last_error()
        assert fn(256, 0, 256, 0, 4, 3, 16, 16, 8, 0, None) == -1 and name.encode() in lib.dvt_last_error()
        assert fn(256, 0, 256, 0, 4, 3, 20, 16, 8, 2, None) == -1 and b"divisible" in lib.dvt_last_error()
        assert fn(256, 0, 256, 0, 4, 3, 16, 20, 8, 2, None) == -1 and b"divisible" in lib.dvt_last_error()
        assert fn(256, 0, 256, 0, 0, 3, 16, 16, 8, 2, None) == 0                   # no frames: nothing is launched
    # the per-frame pair is the same entry at pt = 1, under its own names and without the pt argument
    for name in ("dvt_patchify", "dvt_patchify_bwd"):
        assert name in _lib.SIGNATURES and len(_lib.SIGNATURES[name][1]) == 10
        fn = getattr(lib, name)
        assert fn(None, 0, None, 0, 4, 3, 16, 16, 8, None) == -1 and lib.dvt_last_error().startswith(name.encode() + b":")
        assert fn(256, 0, 256, 0, 4, 3, 20, 16, 8, None) == -1 and b"divisible" in lib.dvt_last_error()
        assert fn(256, 0, 256, 0, 4, 3, 16, 20, 8, None) == -1 and b"divisible" in lib.dvt_last_error()
        assert lib.dvt_last_error().startswith(name.encode() + b":")
        assert fn(256, 0, 256, 0, 0, 3, 16, 16, 8, None) == 0
