"""AutoAugment on the GPU (csrc/autoaugment.hip, dvt_frames_autoaugment, input_stage.AutoAugment) against the Pillow-written
fixture and tests/autoaugment_ref.py, compared with torch.equal -- uint8 and fp32 exactly, bf16 / fp16 against the fp32
expectation rounded to the format.

A workgroup walks the H x W pixels of its sample in strides of its 1024 threads: 37 x 53 = 1961 pixels end in a partial stride,
224 x 224 = 49 x 1024 fills the LDS image the kernel was sized for.  A launch carries 48 samples: the batches of 50 here take two."""
import numpy as np
import pytest
import torch

from tests import augment_ref as A
from tests import autoaugment_ref as R
from tests.test_autoaugment_cpu import CASES, SIZES, case_slot
from tests.util import golden

pytestmark = pytest.mark.gpu

MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
IDENT = [0] * 8


def _check(frames, table, u8, f32, mean=MEAN, std=STD):
    """All four destination formats of one call against the expected uint8 [N, H, W, 3] / float32 [N, 3, H, W]."""
    from dvt_amd import ops
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    table = torch.as_tensor(np.asarray(table), dtype=torch.int32).reshape(len(frames), 2, 8)
    exp = torch.from_numpy(np.ascontiguousarray(f32))
    got8 = ops.frames_autoaugment(dev, table, out_dtype=torch.uint8)
    assert got8.shape == frames.shape and torch.equal(got8.cpu(), torch.from_numpy(np.ascontiguousarray(u8)))
    got = ops.frames_autoaugment(dev, table, mean, std, torch.float32)
    assert got.shape == (len(frames), 3) + frames.shape[1:3] and torch.equal(got.cpu(), exp)
    for dt in (torch.bfloat16, torch.float16):
        got16 = ops.frames_autoaugment(dev, table, mean, std, dt)
        assert got16.dtype == dt and torch.equal(got16.cpu(), exp.to(dt))


@pytest.mark.parametrize("size", SIZES)
def test_every_fixture_case_in_either_slot(device, size):
    """Sample 2 i applies case i as the first operation (source in global memory, result to LDS) and nothing second; sample
    2 i + 1 applies nothing first and case i second (source in LDS, result to the destination)."""
    g = golden("autoaugment.npz")
    frame = g[size + ":frame"]
    H, W, _ = frame.shape
    table, u8, f32 = [], [], []
    for case in CASES:
        s = case_slot(case, H, W)
        table += [[s, IDENT], [IDENT, s]]
        u8 += [g[f"{size}:{case}:u8"]] * 2
        f32 += [g[f"{size}:{case}:f32"]] * 2
    assert len(table) == 50
    _check(np.stack([frame] * 50), table, np.stack(u8), np.stack(f32), g["mean"], g["std"])


def test_all_sub_policies_with_both_sign_pairs(device):
    """The 25 sub-policies of the ImageNet policy, both operations applied, signs (0, 0) and (1, 1), one frame each: the
    second operation reads the first one's result for every kind of pair (statistics after geometry, a blend after a blend,
    tables after tables ...)."""
    H, W = 37, 53
    rng = np.random.default_rng(61)
    frames = rng.integers(0, 256, (50, H, W, 3), dtype=np.uint8)
    frames[::5] = golden("autoaugment.npz")["37x53:frame"]                  # uneven histograms as well as flat ones
    table = [[R.policy_slot(sub[0], sign, H, W), R.policy_slot(sub[1], sign, H, W)] for sub in R.IMAGENET for sign in (0, 1)]
    u8 = R.apply_table(frames, table)
    assert sum(not np.array_equal(a, b) for a, b in zip(u8, frames)) >= 48   # (Color at bin 0 and Rotate at 0 degrees change nothing)
    _check(frames, table, u8, R.normalize(u8, MEAN, STD))


def test_two_identities_give_the_bits_of_frames_augment(device):
    from dvt_amd import ops
    rng = np.random.default_rng(67)
    frames = torch.from_numpy(rng.integers(0, 256, (3, 37, 53, 3), dtype=np.uint8)).cuda()
    crop = [(0, 0, 0, 37, 53, 0, 0), (2, 5, 7, 20, 31, 1, 0), (1, 3, 0, 30, 53, 0, 1)]
    u8 = ops.frames_augment(frames, crop, (24, 29), out_dtype=torch.uint8)
    ident = torch.zeros(3, 2, 8, dtype=torch.int32)
    assert torch.equal(ops.frames_autoaugment(u8, ident, out_dtype=torch.uint8), u8)
    for dt in (torch.float32, torch.bfloat16, torch.float16):
        direct = ops.frames_augment(frames, crop, (24, 29), MEAN, STD, dt)
        assert torch.equal(ops.frames_autoaugment(u8, ident, MEAN, STD, dt), direct)


def test_full_lds_image_224(device):
    """224 x 224: the largest image of the reference and the one the LDS budget was set for."""
    H = W = 224
    rng = np.random.default_rng(71)
    frames = rng.integers(0, 256, (5, H, W, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    frames[1] = np.stack([yy, 40 + xx // 4, (yy + xx) // 2], -1).astype(np.uint8)
    m = lambda op, mid, sign: R.slot(op, R.magnitude(op, mid, sign, H, W), H, W)  # noqa: E731
    table = [[m("Rotate", 8, 1), m("Equalize", None, 1)], [m("Color", 4, 0), m("Contrast", 8, 1)],
             [m("Sharpness", 7, 1), m("Invert", None, 1)], [m("ShearX", 5, 0), m("Equalize", None, 1)], [IDENT, IDENT]]
    u8 = R.apply_table(frames, table)
    assert np.array_equal(u8[4], frames[4])
    _check(frames, table, u8, R.normalize(u8, MEAN, STD))


def test_an_image_above_the_lds_budget_is_refused(device):
    from dvt_amd import ops
    frames = torch.zeros(1, 231, 231, 3, dtype=torch.uint8, device="cuda")    # 160,083 bytes > 160,000
    with pytest.raises(RuntimeError, match=r"status -2.*dvt_frames_autoaugment.*LDS"):
        ops.frames_autoaugment(frames, torch.zeros(1, 2, 8, dtype=torch.int32), MEAN, STD, torch.float32)
    with pytest.raises(RuntimeError, match=r"status -1.*sample 0 slot 1.*op 15"):
        ops.frames_autoaugment(frames[:, :20, :20].contiguous(), [[IDENT, [15] + [0] * 7]], MEAN, STD, torch.float32)
    with pytest.raises(ValueError, match="host"):
        ops.frames_autoaugment(frames, torch.zeros(1, 2, 8, dtype=torch.int32, device="cuda"), MEAN, STD, torch.float32)
    fits = torch.zeros(1, 230, 231, 3, dtype=torch.uint8, device="cuda")      # 159,390 bytes: the largest LDS image used here
    out = ops.frames_autoaugment(fits, [[[R.OP_ID["Invert"]] + [0] * 7, IDENT]], out_dtype=torch.uint8)
    assert bool((out == 255).all())


def test_train_transform_autoaugment_end_to_end(device):
    from dvt_amd.input_stage import train_transform_autoaugment
    rng = np.random.default_rng(73)
    frames = rng.integers(0, 256, (2, 4, 45, 80, 3), dtype=np.uint8)
    t = train_transform_autoaugment(torch.float32, generator=torch.Generator().manual_seed(7))
    out = t(torch.from_numpy(frames).cuda())
    assert out.shape == (2, 4, 3, 224, 224) and out.dtype == torch.float32
    crop, policy = t.last_params
    assert crop is t.first.last_params and policy is t.second.last_params
    assert crop.shape == (8, 7) and policy.shape == (8, 2, 8) and policy.dtype == torch.int32
    assert int((policy[:, :, 0] != 0).sum()) >= 4                            # seed 7 applies operations
    u8 = A.augment_u8(frames.reshape(8, 45, 80, 3), crop.numpy(), 224, 224)
    ref = R.normalize(R.apply_table(u8, policy.numpy()), MEAN, STD)
    assert torch.equal(out.cpu().reshape(8, 3, 224, 224), torch.from_numpy(ref))
    # index=: two views of one frame and a frame of the other clip; passed tables reproduce the call
    views = t(torch.from_numpy(frames).cuda(), index=[3, 3, 6])
    crop, policy = t.last_params
    assert views.shape == (3, 3, 224, 224) and crop[:, 0].tolist() == [3, 3, 6]
    again = t(torch.from_numpy(frames).cuda(), params=crop, policy_params=policy)
    assert torch.equal(views, again)
    u8 = A.augment_u8(frames.reshape(8, 45, 80, 3), crop.numpy(), 224, 224)
    assert torch.equal(views.cpu(), torch.from_numpy(R.normalize(R.apply_table(u8, policy.numpy()), MEAN, STD)))
