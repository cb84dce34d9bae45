"""The device-side training augmentations (MMX_Frame_dl.py:63-71, :81-88) on the GPU: dvt_frames_augment and
dvt_frames_erase against the Pillow-written fixture and tests/augment_ref.py, compared with torch.equal -- uint8 and fp32
exactly, bf16 against the fp32 expectation rounded to bf16.

The fused kernel gives a workgroup a band of 16 output rows (fewer only where the LDS budget asks for it).  Of the
fixture's output heights, 24 (16 + 8), 40 (16 + 16 + 8) and 17 (16 + 1) cross band seams and end in a partial band;
8 is a single partial band."""
import numpy as np
import pytest
import torch

from tests import augment_ref as R
from tests.util import golden

pytestmark = pytest.mark.gpu

SIZES = ("37x53", "48x64")
TAGS = ("whole", "pixel_first", "pixel_last", "interior_up", "wide_down", "tall_right", "down_up", "identity")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def _check(frames, table, out_h, out_w, u8, f32, mean=MEAN, std=STD):
    """All three destination formats of one call against the expected uint8 [N, h, w, 3] / float32 [N, 3, h, w]."""
    from dvt_amd import ops
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    table = torch.as_tensor(np.asarray(table), dtype=torch.int32)
    exp = torch.from_numpy(np.ascontiguousarray(f32))
    got8 = ops.frames_augment(dev, table, (out_h, out_w), out_dtype=torch.uint8)
    assert got8.shape == (len(table), out_h, out_w, 3) and torch.equal(got8.cpu(), torch.from_numpy(np.ascontiguousarray(u8)))
    got = ops.frames_augment(dev, table, (out_h, out_w), mean, std, torch.float32)
    assert got.shape == (len(table), 3, out_h, out_w) and torch.equal(got.cpu(), exp)
    got16 = ops.frames_augment(dev, table, (out_h, out_w), mean, std, torch.bfloat16)
    assert torch.equal(got16.cpu(), exp.to(torch.bfloat16))


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("tag", TAGS)
def test_resample_cases_with_every_flip(device, size, tag):
    g = golden("augment.npz")
    key = f"{size}:{tag}"
    out_h, out_w = (int(v) for v in g[key + ":size"])
    table = g[key + ":table"]
    assert sorted((int(r[5]), int(r[6])) for r in table) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    _check(g[size + ":frames"], table, out_h, out_w, g[key + ":u8"], g[key + ":f32"], g["mean"], g["std"])


@pytest.mark.parametrize("size", SIZES)
def test_mixed_batch_with_shuffled_sources(device, size):
    """Every window of the fixture in one batch of 40 x 23 outputs (two and a half bands), flips and source frames drawn
    per sample, so that samples share frames and neighbours differ in scale, tap count and window."""
    g = golden("augment.npz")
    rng = np.random.default_rng(23)
    rows = []
    for tag in TAGS:
        for _ in range(2):
            _, top, left, h, w, _, _ = (int(v) for v in g[f"{size}:{tag}:table"][0])
            rows.append((int(rng.integers(0, 3)), top, left, h, w, int(rng.integers(0, 2)), int(rng.integers(0, 2))))
    rows += [rows[0], rows[0][:5] + (1 - rows[0][5], rows[0][6])]          # two views of one frame and window
    table = np.array(rows, np.int32)[rng.permutation(len(rows))]
    assert len(set(table[:, 0])) == 3 and len(table) > len(set(table[:, 0]))
    frames = g[size + ":frames"]
    u8 = R.augment_u8(frames, table, 40, 23)
    _check(frames, table, 40, 23, u8, R.normalize(u8, MEAN, STD))


def test_reference_sized_frame_full_height_window(device):
    """360 x 640 -> 224 x 224 with full-height windows: the tallest LDS band the reference's sizes need (scale 360 / 224
    in the vertical pass), beside the whole frame (7 horizontal taps) and a small window that is enlarged."""
    rng = np.random.default_rng(31)
    frames = rng.integers(0, 256, (2, 360, 640, 3), dtype=np.uint8)
    table = [(1, 0, 100, 360, 480, 0, 1), (0, 0, 0, 360, 640, 1, 0), (1, 201, 333, 97, 130, 1, 1)]
    u8 = R.augment_u8(frames, table, 224, 224)
    _check(frames, table, 224, 224, u8, R.normalize(u8, MEAN, STD))


def test_band_of_one_row_where_the_lds_budget_asks_for_it(device):
    """600 rows squeezed to 16 at 256 output columns: a band of 16 output rows would need the whole window in LDS, a band of
    two 114 rows of 768 bytes; the launcher falls back to one output row per workgroup (76 rows, 57 KiB)."""
    rng = np.random.default_rng(37)
    frames = rng.integers(0, 256, (1, 600, 8, 3), dtype=np.uint8)
    table = [(0, 0, 0, 600, 8, 0, 0), (0, 7, 1, 590, 5, 1, 1)]
    u8 = R.augment_u8(frames, table, 16, 256)
    _check(frames, table, 16, 256, u8, R.normalize(u8, MEAN, STD))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_erase_rectangles_and_nothing_else(device, dtype):
    from dvt_amd import ops
    H, W = 21, 30
    rng = np.random.default_rng(41)
    x = torch.from_numpy(rng.standard_normal((8, 3, H, W)).astype(np.float32)).to(dtype)
    table = [(0, 0, 4, 5), (0, W - 7, 3, 7), (H - 2, 0, 2, 9), (H - 6, W - 4, 6, 4),       # the four corners
             (10, 17, 1, 1), (0, 0, 0, 0), (0, 0, H - 1, W - 1), (1, 1, H - 1, W - 1)]
    value = (0.5, -1.25, 3.0)
    ref = torch.from_numpy(R.erase(x.float().numpy(), table, value)).to(dtype)
    got = x.cuda()
    assert ops.frames_erase(got, table, value) is got
    got = got.cpu()
    assert torch.equal(got, ref)
    assert torch.equal(got[5], x[5])                                       # the h == 0 row: bit-identical
    outside = ref == x                                                     # (a fill may coincide with a value: still equal)
    assert torch.equal(got[outside], x[outside])
    zero = ops.frames_erase(x.cuda(), table)                               # the default fill
    assert torch.equal(zero.cpu(), torch.from_numpy(R.erase(x.float().numpy(), table)).to(dtype))


def test_train_transform_wrapper(device):
    from dvt_amd.input_stage import train_transform
    rng = np.random.default_rng(43)
    frames = rng.integers(0, 256, (2, 14, 45, 80, 3), dtype=np.uint8)
    t = train_transform(torch.float32, generator=torch.Generator().manual_seed(7))
    out = t(torch.from_numpy(frames).cuda())
    assert out.shape == (2, 14, 3, 224, 224) and out.dtype == torch.float32
    p = t.last_params
    assert p.shape == (28, 7) and p.dtype == torch.int32 and p[:, 0].tolist() == list(range(28))
    ref = R.augment(frames.reshape(28, 45, 80, 3), p.numpy(), 224, 224, MEAN, STD)
    assert torch.equal(out.cpu().reshape(28, 3, 224, 224), torch.from_numpy(ref))
    # one random frame of each clip, twice (two views): [N] positions among the flattened frames, a passed table
    index = [3, 3, 20, 27]
    views = t(torch.from_numpy(frames).cuda(), index=index)
    assert views.shape == (4, 3, 224, 224) and t.last_params[:, 0].tolist() == index
    again = t(torch.from_numpy(frames).cuda(), params=t.last_params)
    assert torch.equal(views, again)
    assert torch.equal(views.cpu(), torch.from_numpy(R.augment(frames.reshape(28, 45, 80, 3), t.last_params.numpy(), 224, 224,
                                                               MEAN, STD)))


def test_train_vid_frame_wrapper(device):
    from oracle import input_stage as I
    from dvt_amd.input_stage import KINETICS_MEAN, KINETICS_STD, train_vid_frame
    rng = np.random.default_rng(47)
    frames = rng.integers(0, 256, (2, 12, 45, 80, 3), dtype=np.uint8)
    t = train_vid_frame(torch.float32, generator=torch.Generator().manual_seed(3))
    out = t(torch.from_numpy(frames).cuda())
    assert out.shape == (2, 12, 3, 112, 112)
    p = t.second.last_params
    assert p.shape == (24, 4) and 0 < int((p[:, 2] != 0).sum()) < 24       # p = 0.5 over 24 frames, seed 3
    ref = R.erase(I.preprocess_frames(frames.reshape(24, 45, 80, 3), 120, 112, KINETICS_MEAN, KINETICS_STD), p.numpy())
    assert torch.equal(out.cpu().reshape(24, 3, 112, 112), torch.from_numpy(ref))


def test_bad_inputs_raise_before_any_launch(device):
    from dvt_amd import ops
    from dvt_amd.input_stage import RandomErasing, RandomResizedCropFlip
    frames = torch.zeros(2, 20, 30, 3, dtype=torch.uint8, device="cuda")
    row = [(0, 0, 0, 4, 4, 0, 0)]
    with pytest.raises(ValueError, match="uint8"):
        RandomResizedCropFlip(8)(frames.float())
    with pytest.raises(ValueError, match="host"):
        RandomResizedCropFlip(8)(frames, params=torch.tensor(row, dtype=torch.int32, device="cuda"))
    with pytest.raises(ValueError, match="host"):
        ops.frames_erase(torch.zeros(1, 3, 8, 8, device="cuda"), torch.zeros(1, 4, dtype=torch.int32, device="cuda"))
    with pytest.raises(RuntimeError, match="row 1.*leaves"):               # validated in C, before the first launch
        ops.frames_augment(frames, row + [(1, 10, 0, 11, 4, 0, 0)], 8, MEAN, STD, torch.float32)
    with pytest.raises(RuntimeError, match="row 0.*leaves"):
        RandomErasing()(torch.zeros(1, 3, 8, 8, device="cuda"), params=[(0, 0, 9, 1)])
    with pytest.raises(ValueError, match="LDS"):
        ops.frames_augment(torch.zeros(1, 4000, 8, 3, dtype=torch.uint8, device="cuda"), [(0, 0, 0, 4000, 8, 0, 0)], (8, 1024),
                           MEAN, STD, torch.float32)
