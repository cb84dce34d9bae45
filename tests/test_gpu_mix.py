"""csrc/mix.hip on the GPU: ops.clips_mix, ops.targets_mix and ops.ce_soft_* called directly and judged against the float64
statements of tests/mix_ref.py -- copies and untouched samples with torch.equal, everything inexact under the rule of
tests/rowwise_ref.py (4 x the fp32 chain's own error plus one fp32 ulp; a 16-bit output is the float64 result rounded to
the dtype or a neighbouring value) -- and the surfaces built on them: input_stage.Mixup, FrameTransformer(mix=),
BasicMLP with a smoothed loss.  Shapes are the smallest that reach each path: samples that start off their 16-byte
lines (element accesses), runs with a head and a tail, more than one workgroup tile, more rows than one launch carries."""

import pytest
import torch

from tests import mix_ref as MR
from tests import rowwise_ref as R
from tests.guards import guarded, poisoned

pytestmark = pytest.mark.gpu

DT = ["fp32", "bf16", "fp16"]
SENTINEL = 777.0


@pytest.fixture(scope="module")
def dvt(device):
    import dvt_amd
    dvt_amd._lib.load()
    return dvt_amd


def _flip(B):
    return list(range(B - 1, -1, -1))


def _table(partner, kinds, boxes=None):
    boxes = boxes or [(0, 0, 0, 0, 0, 0)] * len(partner)
    return torch.tensor([[p, k, *b] for p, k, b in zip(partner, kinds, boxes)], dtype=torch.int32)


def _clip(shape, name, seed):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(shape, generator=g, dtype=torch.float64) * 1.5 + 0.25).to(R.DTYPES[name])


def _carved(x, device):
    """x on the device inside a sentinel-filled buffer, 16 elements from its start -> (view, check of the bytes around it)"""
    n = x.numel()
    buf = torch.full((n + 80,), SENTINEL, dtype=x.dtype, device=device)
    view = buf[16:16 + n].view(x.shape)
    view.copy_(x)

    def check():
        assert bool((buf[:16] == SENTINEL).all()) and bool((buf[16 + n:] == SENTINEL).all()), "bytes around the tensor were written"
    return view, check


def _run_both(ops, device, x, table, lam):
    """in place and out of place, each inside sentinels; the two must agree bit for bit -> the result on the CPU"""
    a, chk_a = _carved(x, device)
    assert ops.clips_mix(a, table, lam) is a
    src, chk_s = _carved(x, device)
    dst, chk_d = _carved(torch.full_like(x, SENTINEL), device)
    assert ops.clips_mix(src, table, lam, out=dst) is dst
    torch.cuda.synchronize()
    chk_a(); chk_s(); chk_d()
    assert torch.equal(src.cpu(), x), "out of place wrote its input"
    assert torch.equal(a.cpu(), dst.cpu()), "in place and out of place differ"
    return dst.cpu()


def _judge(got, x, table, lam, tag):
    ref = MR.clips_mix(x.double(), table, lam)
    chain = MR.clips_mix(x.float(), table, lam)
    mag = torch.maximum(x.double().abs(), x.double()[table[:, 0].long()].abs())
    R.assert_close(got, ref, chain, mag, tag)
    lam32 = torch.as_tensor(lam, dtype=torch.float32)
    for i in range(x.shape[0]):
        row = table[i].tolist()
        if not MR.changes(row, i, lam32[i]):
            assert torch.equal(got[i], x[i]), f"{tag}: sample {i} must be bit-identical to the input"
        elif row[1] == MR.KIND_CUTMIX:
            assert torch.equal(got[i], ref[i].to(got.dtype)), f"{tag}: sample {i} is a copy and must be exact"


# ---------------------------------------------------------------- mixup
@pytest.mark.parametrize("name", DT)
def test_mixup_unaligned(dvt, device, name):
    """315 elements per sample: 16-bit samples start off their 16-byte lines and the members of a pair sit differently in
    theirs (element accesses); an fp32 pair (0, 4) sits alike (vector slots and a 3-element tail); sample 2 pairs with itself"""
    x = _clip((5, 3, 3, 5, 7), name, 1)
    table = _table(_flip(5), [1] * 5)
    lam = [0.3, 1.0, 0.7, 0.0, 0.5]
    got = _run_both(dvt.ops, device, x, table, lam)
    _judge(got, x, table, lam, f"mixup {name} unaligned")
    assert torch.equal(got[1], x[1]) and torch.equal(got[2], x[2])


@pytest.mark.parametrize("shape", [(4, 2, 3, 8, 16), (2, 1, 3, 64, 64), (3, 1, 3, 5, 8)], ids=["768", "12288", "120-odd-B"])
@pytest.mark.parametrize("name", DT)
def test_mixup_aligned(dvt, device, name, shape):
    """samples that are whole 16-byte lines; 12288 elements are more than one workgroup tile of 1024 slots in fp32"""
    x = _clip(shape, name, 2)
    B = shape[0]
    table = _table(_flip(B), [1] * B)
    lam = [0.25, 0.6, 0.9, 0.1][:B]
    got = _run_both(dvt.ops, device, x, table, lam)
    _judge(got, x, table, lam, f"mixup {name} {shape}")


# ---------------------------------------------------------------- cutmix
BOXES = {"full": (0, 3, 0, 9, 0, 13), "corner00": (0, 3, 0, 1, 0, 1), "corner01": (0, 3, 0, 1, 12, 13),
         "corner10": (0, 3, 8, 9, 0, 1), "corner11": (0, 3, 8, 9, 12, 13), "odd": (0, 3, 2, 7, 3, 10),
         "full-width": (0, 3, 2, 6, 0, 13), "one-frame": (1, 2, 1, 8, 2, 11), "whole-frames": (1, 3, 0, 9, 0, 13),
         "empty": (0, 3, 4, 4, 2, 9)}


@pytest.mark.parametrize("box", list(BOXES))
@pytest.mark.parametrize("name", DT)
def test_cutmix_exact(dvt, device, name, box):
    x = _clip((4, 3, 3, 9, 13), name, 3)
    table = _table(_flip(4), [2] * 4, [BOXES[box]] * 4)
    got = _run_both(dvt.ops, device, x, table, [0.5] * 4)
    assert torch.equal(got, MR.clips_mix(x, table, [0.5] * 4)), f"cutmix {name} {box}"
    _judge(got, x, table, [0.5] * 4, f"cutmix {name} {box}")


@pytest.mark.parametrize("name", DT)
def test_cutmix_elem_boxes_and_mixed_kinds(dvt, device, name):
    """'elem' tables: the members of a pair carry different (overlapping, nested, disjoint) boxes, or one is mixed and the
    other cut, or only one of them changes"""
    x = _clip((8, 3, 3, 9, 13), name, 4)
    kinds = [2, 2, 1, 2, 0, 2, 2, 2]
    boxes = [(0, 3, 1, 6, 2, 9), (0, 2, 0, 9, 0, 13), (0, 0, 0, 0, 0, 0), (0, 3, 0, 4, 0, 5), (0, 0, 0, 0, 0, 0),
             (1, 3, 2, 8, 4, 12), (1, 2, 3, 5, 4, 8), (0, 3, 4, 9, 5, 13)]
    table = _table(_flip(8), kinds, boxes)
    lam = [0.5, 0.5, 0.35, 0.5, 1.0, 0.5, 0.5, 0.5]
    got = _run_both(dvt.ops, device, x, table, lam)
    _judge(got, x, table, lam, f"elem {name}")


@pytest.mark.parametrize("name", ["fp32", "bf16"])
def test_chunking(dvt, device, name):
    """more samples than two launches carry rows.  Kinds alternate leave / mixup / leave / cutmix: under the flip every
    second pair changes nothing and makes no row, so in place the whole batch fits one launch while out of place, where
    every sample is written, it takes three; with every pair mixed the in-place rows need a second launch too"""
    B = 2 * dvt.ops.MIX_ROWS_PER_LAUNCH + 3
    x = _clip((B, 1, 3, 4, 4), name, 5)
    kinds = [(0, 1, 0, 2)[i % 4] for i in range(B)]
    table = _table(_flip(B), kinds, [(0, 1, 1, 3, 0, 3)] * B)
    lam = [0.25 + 0.5 * (i % 3) / 2 for i in range(B)]
    got = _run_both(dvt.ops, device, x, table, lam)
    _judge(got, x, table, lam, f"chunking {name}")
    every = _table(_flip(B), [1] * B)                                # every pair changes: more rows than one launch
    got = _run_both(dvt.ops, device, x, every, lam)
    _judge(got, x, every, lam, f"chunking, all mixed {name}")


@pytest.mark.parametrize("name", DT)
def test_roll_partner(dvt, device, name):
    x = _clip((4, 2, 3, 6, 8), name, 6)
    roll = [1, 2, 3, 0]
    table = _table(roll, [1, 2, 1, 2], [(0, 2, 1, 5, 2, 7)] * 4)
    lam = [0.4, 0.5, 0.8, 0.5]
    src = x.to(device)
    dst, chk = poisoned(tuple(x.shape), x.dtype, device)
    dvt.ops.clips_mix(src, table, lam, out=dst)
    chk()
    _judge(dst.cpu(), x, table, lam, f"roll {name}")
    with pytest.raises(ValueError, match="involution"):
        dvt.ops.clips_mix(src, table, lam)
    assert torch.equal(src.cpu(), x)
    with pytest.raises(ValueError, match="host array"):
        dvt.ops.clips_mix(src, table.to(device), lam)
    with pytest.raises(ValueError, match="contiguous"):
        dvt.ops.clips_mix(src.transpose(3, 4), table, lam, out=dst)
    with pytest.raises(ValueError, match="host array"):
        dvt.ops.clips_mix(src, table, torch.tensor(lam, device=device), out=dst)
    y = torch.zeros(4, 5, device=device)
    with pytest.raises(ValueError, match="host array"):
        dvt.ops.targets_mix(table.to(device), lam, y=y)
    with pytest.raises(ValueError, match="host array"):
        dvt.ops.targets_mix(table, torch.tensor(lam, device=device), y=y)


def test_folded_middle_dimensions(dvt, device):
    """[B, 3, 2, C, H, W] is T = 6"""
    x = _clip((2, 3, 2, 3, 6, 8), "bf16", 7)
    table = _table([1, 0], [2, 1], [(2, 5, 1, 4, 0, 8), (0,) * 6])
    got = dvt.ops.clips_mix(x.to(device), table, [0.5, 0.25]).cpu()
    flat = x.view(2, 6, 3, 6, 8)
    _judge(got.view(2, 6, 3, 6, 8), flat, table, [0.5, 0.25], "folded")


# ---------------------------------------------------------------- targets
def _judge_targets(got, t, table, lam, tag):
    ref = MR.targets_mix(t.double(), table, lam)
    chain = MR.targets_mix(t.float(), table, lam)
    nan = torch.isnan(ref)
    assert torch.equal(torch.isnan(got), nan), f"{tag}: NaN rows"
    keep = ~nan.any(1)
    R.assert_close(got[keep], ref[keep], chain[keep], 1.0, tag)


def test_targets_mix(dvt, device):
    ops = dvt.ops
    g = torch.Generator().manual_seed(8)
    table = _table(_flip(5), [1, 2, 0, 1, 2])
    lam = [0.3, 1.0, 1.0, 0.0, 0.625]
    y = (torch.rand(5, 19, generator=g) < 0.3).float()
    with guarded(ops):
        got = ops.targets_mix(table, lam, y=y.to(device))
    _judge_targets(got.cpu(), y, table, lam, "multi-hot")
    assert torch.equal(got[1].cpu(), y[1]) and torch.equal(got[2].cpu(), y[2])
    labels = torch.tensor([3, 0, 6, 2, 5])
    with guarded(ops):
        got = ops.targets_mix(table, lam, labels=labels.to(device), num_classes=7, smoothing=0.1)
    _judge_targets(got.cpu(), MR.label_rows(labels, 7, 0.1, torch.float32), table, lam, "labels, smoothing 0.1")
    hard = ops.targets_mix(table, lam, labels=labels.to(device), num_classes=7).cpu()
    onehot = torch.nn.functional.one_hot(labels, 7).float()
    assert torch.equal(hard[1], onehot[1]) and torch.equal(hard[2], onehot[2])
    _judge_targets(hard, onehot, table, lam, "labels, no smoothing")
    # a label outside [0, C): its row is NaN, so is the row that mixes it in; every other row is as without it
    bad = labels.clone()
    bad[1] = 7                                                     # row 1 (lam 1) is NaN; its partner, row 3, has lam 0: NaN too
    got = ops.targets_mix(table, lam, labels=bad.to(device), num_classes=7, smoothing=0.1).cpu()
    good = ops.targets_mix(table, lam, labels=labels.to(device), num_classes=7, smoothing=0.1).cpu()
    assert torch.isnan(got[1]).all() and torch.isnan(got[3]).all()
    assert torch.equal(got[[0, 2, 4]], good[[0, 2, 4]])
    bad = labels.clone()
    bad[3] = -1                                                    # its partner, row 1, has lam 1 and does not read it
    got = ops.targets_mix(table, lam, labels=bad.to(device), num_classes=7, smoothing=0.1).cpu()
    assert torch.isnan(got[3]).all() and torch.equal(got[[0, 1, 2, 4]], good[[0, 1, 2, 4]])
    big = 300                                                      # more rows than one launch carries
    yb = torch.rand(big, 5, generator=g)
    tb = _table(_flip(big), [1] * big)
    lb = torch.rand(big, generator=g).tolist()
    _judge_targets(ops.targets_mix(tb, lb, y=yb.to(device)).cpu(), yb, tb, lb, "300 rows")


# ---------------------------------------------------------------- soft-target cross-entropy
def _soft_case(M, C, dtype, seed):
    g = torch.Generator().manual_seed(seed)
    logits = (torch.randn(M, C, generator=g, dtype=torch.float64) * 2).to(dtype)
    t = torch.softmax(torch.randn(M, C, generator=g, dtype=torch.float64) * 2, 1).float()         # Dirichlet-like rows
    t[0] = 0.0                                                     # an all-zero row
    t[M // 2] = 2.0 * t[M // 2] if M > 1 else t[M // 2]            # a row that sums to 2
    return logits, t


def _soft_run(ops, device, logits, t, tag, ld=None):
    M, C = logits.shape
    if ld is None:
        dev = logits.to(device)
    else:
        buf, chk = poisoned((M, ld), logits.dtype, device)
        buf[:, :C] = logits.to(device)
        dev = buf[:, :C]
    td = t.to(device)
    with guarded(ops):
        loss, lse = ops.ce_soft_fwd(dev, td)
    loss2, lse2 = ops.ce_soft_fwd(dev, td)
    assert torch.equal(loss, loss2) and torch.equal(lse, lse2), f"{tag}: two calls differ"
    loss, lse = loss.cpu(), lse.cpu()
    rl, rlse, rts = MR.ce_soft(logits.double(), t.double())
    cl, clse, cts = MR.ce_soft(logits.float(), t)
    xmag = logits.double().abs().max(1).values
    R.assert_close(lse[:M], rlse, clse, xmag, f"lse {tag}")
    R.assert_close(lse[M:], rts, cts, t.double().abs().max(1).values, f"target sums {tag}")
    R.assert_close(loss, rl.reshape(1), cl.reshape(1), float(xmag.max()) * max(1.0, float(rts.max())), f"loss {tag}")
    gloss = torch.tensor([1.7])
    handed = torch.cat([clse, cts])
    with guarded(ops):
        dl = ops.ce_soft_bwd(dev, td, handed.to(device), gloss.to(device))
    dl2 = ops.ce_soft_bwd(dev, td, handed.to(device), gloss.to(device))
    assert torch.equal(dl, dl2), f"{tag}: two backward calls differ"
    if ld is not None:
        chk()
    ref = MR.ce_soft_bwd(logits.double(), t.double(), clse.double(), cts.double(), gloss.double())
    chain = MR.ce_soft_bwd(logits.float(), t, clse, cts, gloss)
    R.assert_close(dl.cpu(), ref, chain, float(gloss) / M * max(1.0, float(cts.max())), f"dlogits {tag}")
    return loss, lse, dl.cpu()


@pytest.mark.parametrize("name", DT)
def test_ce_soft(dvt, device, name):
    for M in (1, 17, 33):
        for C in (1, 65, 305):
            logits, t = _soft_case(M, C, R.DTYPES[name], M * 1000 + C)
            _soft_run(dvt.ops, device, logits, t, f"{name} M={M} C={C}")


@pytest.mark.parametrize("name", DT)
def test_ce_soft_padded_rows(dvt, device, name):
    for M, C, ld in ((17, 65, 72), (33, 1, 8), (16, 305, 311)):
        logits, t = _soft_case(M, C, R.DTYPES[name], M * 1000 + C + 1)
        _soft_run(dvt.ops, device, logits, t, f"{name} M={M} C={C} ld={ld}", ld=ld)


@pytest.mark.parametrize("name", DT)
def test_ce_soft_one_hot_is_ce_labels(dvt, device, name):
    ops = dvt.ops
    M, C = 17, 65
    g = torch.Generator().manual_seed(9)
    logits = (torch.randn(M, C, generator=g, dtype=torch.float64) * 2).to(R.DTYPES[name])
    labels = torch.randint(0, C, (M,), generator=g)
    onehot = torch.nn.functional.one_hot(labels, C).float()
    loss, lse, dl = _soft_run(ops, device, logits, onehot, f"{name} one-hot")
    hl, hlse = ops.ce_labels_fwd(logits.to(device), labels.to(device))
    assert torch.equal(hlse[:M].cpu(), lse[:M])                   # the same log-sum-exp, in the same order
    rl, _, _ = MR.ce_soft(logits.double(), onehot.double())
    cl, clse, cts = MR.ce_soft(logits.float(), onehot)
    R.assert_close(hl.cpu(), rl.reshape(1), cl.reshape(1), float(logits.double().abs().max()), f"{name} ce_labels loss")
    gloss = torch.tensor([1.7])
    hd = ops.ce_labels_bwd(logits.to(device), labels.to(device), torch.cat([clse, torch.tensor([float(M)])]).to(device),
                           gloss.to(device)).cpu()
    ref = MR.ce_soft_bwd(logits.double(), onehot.double(), clse.double(), cts.double(), gloss.double())
    chain = MR.ce_soft_bwd(logits.float(), onehot, clse, cts, gloss)
    R.assert_close(hd, ref, chain, float(gloss) / M, f"{name} ce_labels dlogits")
    R.assert_close(dl, ref, chain, float(gloss) / M, f"{name} ce_soft dlogits")


def test_soft_target_cross_entropy_autograd(dvt, device):
    """the autograd Function end to end: the loss, and the gradient for an upstream gradient of 1.7 from the forward's own
    saved lse and target sums -- so the fp32 chain is the whole fp32 forward followed by the fp32 backward"""
    F = dvt.functional
    M = 9
    logits, t = _soft_case(M, 21, torch.float32, 11)
    x = logits.to(device).requires_grad_(True)
    td = t.to(device).requires_grad_(True)
    loss = F.soft_target_cross_entropy(x, td)
    gloss = torch.tensor(1.7)
    loss.backward(gloss.to(device))
    assert td.grad is None
    rl, rlse, rts = MR.ce_soft(logits.double(), t.double())
    cl, clse, cts = MR.ce_soft(logits.float(), t)
    xmag = float(logits.double().abs().max())
    R.assert_close(loss.detach().cpu().reshape(1), rl.reshape(1), cl.reshape(1), xmag * max(1.0, float(rts.max())), "autograd loss")
    ref = MR.ce_soft_bwd(logits.double(), t.double(), rlse, rts, gloss.double())
    chain = MR.ce_soft_bwd(logits.float(), t, clse, cts, gloss)
    R.assert_close(x.grad.cpu(), ref, chain, float(gloss) / M * max(1.0, float(rts.max())), "autograd dlogits")
    with pytest.raises(TypeError):
        F.soft_target_cross_entropy(x, torch.zeros(M, dtype=torch.int64, device=device))


# ---------------------------------------------------------------- surfaces
def test_mixup_object_is_ops_with_its_params(dvt, device):
    from dvt_amd.input_stage import Mixup
    ops = dvt.ops
    x = _clip((6, 4, 3, 10, 12), "bf16", 12)
    labels = torch.tensor([0, 4, 2, 2, 1, 3])
    m = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, mode="elem", num_classes=5, generator=torch.Generator().manual_seed(5))
    dev = x.to(device)
    out, mixed = m(dev, labels.to(device))
    assert out is dev and mixed.shape == (6, 5) and mixed.dtype == torch.float32
    table, lam_in, lam_t = m.last_params
    assert set(table[:, 1].tolist()) >= {1, 2}                      # this seed draws both kinds
    by_hand = ops.clips_mix(x.to(device), table, lam_in)
    assert torch.equal(out, by_hand)
    assert torch.equal(mixed, ops.targets_mix(table, lam_t, labels=labels.to(device), num_classes=5, smoothing=0.1))
    # float targets are mixed as they are; a second tensor of another size shares the table, its boxes scaled
    y = (torch.rand(6, 19, generator=torch.Generator().manual_seed(1)) < 0.3).float()
    img = _clip((6, 2, 3, 20, 24), "bf16", 13)
    params = m.last_params
    (a, b), mixed = m((x.to(device), img.to(device)), y.to(device), params=params)
    assert torch.equal(a, by_hand) and torch.equal(mixed, ops.targets_mix(table, lam_t, y=y.to(device)))
    from dvt_amd.input_stage import scale_box
    tab2 = table.clone()
    for i in range(6):
        tab2[i, 2:] = torch.tensor(scale_box(table[i, 2:].tolist(), (4, 10, 12), (2, 20, 24)), dtype=torch.int32)
    assert torch.equal(b, ops.clips_mix(img.to(device), tab2, lam_in))
    _judge(b.cpu(), img, tab2, lam_in, "second tensor")


def _make_ft(mix):
    from dvt_amd.models.frame_transformer import FrameTransformer
    from tests.encoders import PatchLinearEncoder
    torch.manual_seed(1130)
    d, dtype = 64, torch.float32
    cfg = dict(batch_size=2, seq_len=4, cls=1, model="sum", opt="adamW", learning_rate=5e-6, weight_decay=0.09,
               momentum=0.005, d_model=d, tokens=5, frame_len=2, clip_size=16, img_size=32, vid_nhead=2, vid_nhid=96,
               scene_nhead=2, scene_nhid=96, compute_dtype=dtype, encoder_dropout=0.0,
               vid_encoder=PatchLinearEncoder(3, 8, 32, d, dtype), img_encoder=PatchLinearEncoder(3, 8, 32, d, dtype))
    if mix is not None:
        cfg["mix"] = mix
    return FrameTransformer(**cfg).cuda().train()


def test_frame_transformer_mix(dvt, device):
    from dvt_amd.input_stage import Mixup
    g = torch.Generator().manual_seed(3)
    vid = torch.randn(2, 4, 2, 3, 16, 16, generator=g)
    img = torch.randn(2, 4, 3, 32, 32, generator=g)
    target = (torch.rand(2, 19, generator=g) < 0.3).float()
    batch = lambda: (target.cuda(), img.cuda(), vid.cuda())        # noqa: E731  (fresh tensors: the step mixes in place)
    m = Mixup(mixup_alpha=0.8, cutmix_alpha=1.0, generator=torch.Generator().manual_seed(2))
    net = _make_ft(m)
    plain = _make_ft(None)
    assert net.mix is m and plain.mix is None and not hasattr(net.hparams, "mix")
    assert list(net.state_dict()) == list(plain.state_dict())
    loss = net.training_step(batch(), 0)
    table, lam_in, lam_t = m.last_params
    assert int(table[0, 1]) != 0
    t2, i2, v2 = batch()
    (i2, v2), mixed = m((i2, v2), t2, params=m.last_params)
    by_hand, _ = net._loss((mixed, i2, v2))
    assert torch.equal(loss.detach(), by_hand.detach())
    base = plain.training_step(batch(), 0)
    assert float(base.detach()) != float(loss.detach())
    # the metric saw the integer labels, and evaluation does not mix
    draws = m.last_params
    m.last_params = None
    val = net.validation_step(batch(), 0)
    assert m.last_params is None and torch.equal(val.detach(), plain.validation_step(batch(), 0).detach())
    net.eval()
    assert torch.equal(net.training_step(batch(), 0).detach(), plain.eval().training_step(batch(), 0).detach())
    assert m.last_params is None and draws is not None


def test_basic_mlp_label_smoothing(dvt, device):
    from torch import nn
    from dvt_amd.models.basicmlp import BasicMLP
    torch.manual_seed(0)
    net = BasicMLP(dict(input_shape=64, bottle_neck=1024, output_shape=305, batch_size=8, learning_rate=1e-3,
                        aggregation="concat")).cuda()
    g = torch.Generator().manual_seed(4)
    logits = (torch.randn(9, 305, generator=g) * 2)
    labels = torch.randint(0, 305, (9,), generator=g)
    dev = logits.cuda().requires_grad_(True)
    parent = net.criterion(dev, labels.cuda())
    net.loss = nn.CrossEntropyLoss(label_smoothing=0.0)
    assert torch.equal(net.criterion(dev, labels.cuda()), parent)                  # s == 0: the integer-label path, as before
    net.loss = nn.CrossEntropyLoss(label_smoothing=0.1)
    loss = net.criterion(dev, labels.cuda())
    loss.backward()
    rows64 = MR.label_rows(labels, 305, 0.1, torch.float64)
    ref = nn.CrossEntropyLoss(label_smoothing=0.1)(logits.double(), labels)
    chain = MR.ce_soft(logits.float(), MR.label_rows(labels, 305, 0.1, torch.float32))[0]
    # the restatement is torch's loss but for the smoothing constant, which the kernel holds in fp32: |0.1f - 0.1| = 1.5e-9,
    # times a spread of log-probabilities below 40
    assert abs(float(MR.ce_soft(logits.double(), rows64)[0]) - float(ref)) < 40 * 1.5e-9
    R.assert_close(loss.detach().cpu().reshape(1), ref.reshape(1), chain.reshape(1), float(logits.abs().max()), "smoothed loss")
    lr = logits.double().requires_grad_(True)
    nn.CrossEntropyLoss(label_smoothing=0.1)(lr, labels).backward()                # torch's float64 gradient is the reference
    rows32 = MR.label_rows(labels, 305, 0.1, torch.float32)
    _, clse, cts = MR.ce_soft(logits.float(), rows32)
    gchain = MR.ce_soft_bwd(logits.float(), rows32, clse, cts, torch.tensor(1.0))
    R.assert_close(dev.grad.cpu(), lr.grad, gchain, 1.0 / 9, "smoothed dlogits")
    soft = net.loss
    net.loss = nn.CrossEntropyLoss()
    rows = MR.label_rows(labels, 305, 0.1, torch.float32)
    got = net.criterion(dev, rows.cuda())                                          # float [M, C] labels go the same way
    R.assert_close(got.detach().cpu().reshape(1), ref.reshape(1), chain.reshape(1), float(logits.abs().max()), "float labels")
    net.loss = soft
    with pytest.raises(NotImplementedError):
        net.criterion(dev, rows.cuda())
    net.loss = nn.CrossEntropyLoss(label_smoothing=0.1, reduction="sum")
    with pytest.raises(NotImplementedError):
        net.criterion(dev, labels.cuda())
    net.loss = nn.CrossEntropyLoss(label_smoothing=0.1, ignore_index=3)             # every row counts on this path
    with pytest.raises(NotImplementedError, match="ignore_index"):
        net.criterion(dev, labels.cuda())
    net.loss = nn.CrossEntropyLoss(ignore_index=3)                                 # the integer-label path keeps honouring it
    assert torch.isfinite(net.criterion(dev, labels.cuda()))
