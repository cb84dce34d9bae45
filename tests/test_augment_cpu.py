"""Training augmentations of MMX_Frame_dl.py:63-71 / :81-88 without a GPU: the numpy restatement (tests/augment_ref.py)
against the fixture written through Pillow and against the installed Pillow, the host samplers of dvt_amd.input_stage,
and the C surface (declarations, host-side validation of the parameter tables before any HIP call)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from tests import augment_ref as R
from tests.util import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ("37x53", "48x64")
TAGS = ("whole", "pixel_first", "pixel_last", "interior_up", "wide_down", "tall_right", "down_up", "identity")


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("tag", TAGS)
def test_reference_matches_pillow_fixture(size, tag):
    g = golden("augment.npz")
    assert tuple(g["tags"]) == TAGS
    key = f"{size}:{tag}"
    out_h, out_w = (int(v) for v in g[key + ":size"])
    table = g[key + ":table"]
    assert sorted((int(r[5]), int(r[6])) for r in table) == [(0, 0), (0, 1), (1, 0), (1, 1)]
    u8 = R.augment_u8(g[size + ":frames"], table, out_h, out_w)
    assert np.array_equal(u8, g[key + ":u8"])
    f32 = R.augment(g[size + ":frames"], table, out_h, out_w, g["mean"], g["std"])
    assert f32.dtype == np.float32 and np.array_equal(f32, g[key + ":f32"])


def test_fixture_holds_the_many_taps_case():
    from oracle.input_stage import resample_coeffs
    g = golden("augment.npz")
    w = int(g["37x53:wide_down:table"][0][4])
    assert w == 53 and resample_coeffs(w, 8)[2].shape[1] == 15


def test_reference_against_installed_pillow():
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(17)
    for (H0, W0, out) in ((37, 53, 24), (90, 160, 56), (64, 48, 7)):
        frames = rng.integers(0, 256, (2, H0, W0, 3), dtype=np.uint8)
        table = []
        for n in range(8):
            h, w = int(rng.integers(1, H0 + 1)), int(rng.integers(1, W0 + 1))
            table.append((n % 2, int(rng.integers(0, H0 - h + 1)), int(rng.integers(0, W0 - w + 1)), h, w, n & 1, (n >> 1) & 1))
        got = R.augment_u8(frames, table, out, out + 3)
        for n, (f, top, left, h, w, hf, vf) in enumerate(table):
            img = Image.fromarray(frames[f]).crop((left, top, left + w, top + h)).resize((out + 3, out), Image.BILINEAR)
            img = img.transpose(Image.FLIP_LEFT_RIGHT) if hf else img
            img = img.transpose(Image.FLIP_TOP_BOTTOM) if vf else img
            assert np.array_equal(got[n], np.asarray(img)), (H0, W0, table[n])


def test_erase_reference():
    x = np.arange(2 * 3 * 4 * 5, dtype=np.float32).reshape(2, 3, 4, 5)
    y = R.erase(x, [(1, 2, 2, 3), (0, 0, 0, 0)], (7, 8, 9))
    assert np.array_equal(y[1], x[1]) and np.array_equal(y[0, :, 0], x[0, :, 0]) and np.array_equal(y[0, :, :, :2], x[0, :, :, :2])
    assert all((y[0, c, 1:3, 2:5] == 7 + c).all() for c in range(3))


# ---------------------------------------------------------------- samplers
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_resized_crop_windows_lie_inside_the_frame():
    from dvt_amd.input_stage import draw_resized_crop
    g = _gen(3)
    seen = set()
    for H0, W0 in ((45, 80), (360, 640), (100, 10), (7, 7)):
        for _ in range(200):
            top, left, h, w = draw_resized_crop(H0, W0, generator=g)
            assert 1 <= h <= H0 and 1 <= w <= W0 and 0 <= top <= H0 - h and 0 <= left <= W0 - w
            seen.add((H0, W0, top, left, h, w))
    assert len(seen) > 400                                       # windows are drawn, not constant


def test_resized_crop_fallback_branches():
    """scale (4, 4): the target area is 4 x the frame, so w <= W0 and h <= H0 cannot both hold and all 10 tries miss."""
    from dvt_amd.input_stage import draw_resized_crop
    lo, hi = 3.0 / 4.0, 4.0 / 3.0
    # 10 x 100 (H0 x W0): W0 / H0 = 10 > 4/3 -> h = H0, w = round(h * 4/3), centred
    assert draw_resized_crop(10, 100, scale=(4.0, 4.0), generator=_gen(0)) == (0, (100 - 13) // 2, 10, int(round(10 * hi)))
    # 100 x 10: W0 / H0 = 0.1 < 3/4 -> w = W0, h = round(w / (3/4)), centred
    assert draw_resized_crop(100, 10, scale=(4.0, 4.0), generator=_gen(0)) == ((100 - 13) // 2, 0, int(round(10 / lo)), 10)
    # in range: the whole frame
    assert draw_resized_crop(30, 30, scale=(4.0, 4.0), generator=_gen(0)) == (0, 0, 30, 30)


def test_same_seed_same_table_and_flip_extremes():
    from dvt_amd.input_stage import RandomErasing, RandomResizedCropFlip
    a = RandomResizedCropFlip(24, hflip_p=0.3, vflip_p=0.3, generator=_gen(11)).draw(45, 80, range(28))
    b = RandomResizedCropFlip(24, hflip_p=0.3, vflip_p=0.3, generator=_gen(11)).draw(45, 80, range(28))
    c = RandomResizedCropFlip(24, hflip_p=0.3, vflip_p=0.3, generator=_gen(12)).draw(45, 80, range(28))
    assert a.dtype == torch.int32 and a.shape == (28, 7) and torch.equal(a, b) and not torch.equal(a, c)
    assert a[:, 0].tolist() == list(range(28))
    never = RandomResizedCropFlip(24, hflip_p=0.0, vflip_p=0.0, generator=_gen(1)).draw(45, 80, range(64))
    always = RandomResizedCropFlip(24, hflip_p=1.0, vflip_p=1.0, generator=_gen(1)).draw(45, 80, range(64))
    assert not never[:, 5:].any() and always[:, 5:].all()
    assert torch.equal(never[:, 1:5], always[:, 1:5])            # the flip draws do not move the crop draws
    e1, e2 = (RandomErasing(generator=_gen(5)).draw(112, 112, 48) for _ in range(2))
    assert torch.equal(e1, e2) and e1.shape == (48, 4)


def test_erase_rectangles():
    from dvt_amd.input_stage import RandomErasing
    for H, W in ((112, 112), (20, 31)):
        t = RandomErasing(p=1.0, generator=_gen(2)).draw(H, W, 300)
        on = t[t[:, 2] != 0]
        assert len(on) > 250                                       # 10 tries rarely all miss
        assert ((on[:, 2] < H) & (on[:, 3] < W) & (on[:, 2] >= 1) & (on[:, 3] >= 1)).all()
        assert ((on[:, 0] >= 0) & (on[:, 1] >= 0) & (on[:, 0] + on[:, 2] <= H) & (on[:, 1] + on[:, 3] <= W)).all()
        assert not t[t[:, 2] == 0].any()
    assert not RandomErasing(p=0.0, generator=_gen(2)).draw(112, 112, 100).any()
    half = RandomErasing(generator=_gen(4)).draw(112, 112, 400)
    assert 120 < int((half[:, 2] != 0).sum()) < 280                # p = 0.5
    with pytest.raises(NotImplementedError):
        RandomErasing(value="random")


def test_factories():
    from dvt_amd import input_stage as S
    t = S.train_transform(torch.float32)
    assert (t.size, t.hflip_p, t.vflip_p, t.mean, t.std) == (224, 0.3, 0.3, S.IMAGENET_MEAN, S.IMAGENET_STD)
    assert (t.scale, t.ratio) == ((0.08, 1.0), (3.0 / 4.0, 4.0 / 3.0))
    with pytest.raises(NotImplementedError, match="uint8"):
        S.train_transform(torch.float32, auto_augment=True)
    v = S.train_vid_frame(torch.float32)
    assert (v.first.resize, v.first.crop, v.first.mean) == (120, 112, S.KINETICS_MEAN)
    assert (v.second.p, v.second.scale, v.second.ratio, v.second.value) == (0.5, (0.02, 0.33), (0.3, 3.3), (0.0, 0.0, 0.0))


def test_wrappers_refuse_bad_inputs_before_any_launch():
    from dvt_amd import ops
    from dvt_amd.input_stage import RandomResizedCropFlip
    with pytest.raises(ValueError, match="uint8"):
        RandomResizedCropFlip(8)(torch.zeros(1, 20, 30, 3))
    with pytest.raises(ValueError, match="uint8"):
        ops.frames_augment(torch.zeros(1, 20, 30, 3), [(0, 0, 0, 4, 4, 0, 0)], 8, (0, 0, 0), (1, 1, 1), torch.float32)
    with pytest.raises(ValueError, match=r"\[rows, 7\]"):
        ops.frames_augment(torch.zeros(1, 20, 30, 3, dtype=torch.uint8), [(0, 0, 0, 4)], 8, (0, 0, 0), (1, 1, 1), torch.float32)
    with pytest.raises(ValueError, match="table rows"):
        ops.frames_erase(torch.zeros(2, 3, 8, 8), [(0, 0, 1, 1)])


# ---------------------------------------------------------------- C surface
NAMES = ("dvt_frames_augment_workspace_bytes", "dvt_frames_augment", "dvt_frames_erase")


def _lib():
    import dvt_amd
    return dvt_amd._lib.load()


def test_header_declares_the_entry_points():
    import dvt_amd
    header = open(os.path.join(ROOT, "include", "dvt_hip.h")).read()
    for n in NAMES:
        assert re.search(rf"\b{n}\s*\(", header) and n in dvt_amd._lib.SIGNATURES
    assert "MMX_Frame_dl.py:63-71" in header and "MMX_Frame_dl.py" in header and ":81-88" in header
    assert _lib().dvt_version() == 5 and dvt_amd._lib.ABI_VERSION == 5
    assert dvt_amd._lib.ENUMS["dvt_augment_dst"] == {"DVT_AUGMENT_U8_HWC": 8}
    assert dvt_amd._lib.ENUMS["dvt_dtype"] == {"DVT_F32": 0, "DVT_BF16": 1, "DVT_F16": 2}


def _augment(lib, rows, frames=2, H0=20, W0=30, out=8, dst_dtype=0):
    """dvt_frames_augment on dummy non-null device pointers: the table is validated before anything touches them."""
    tab = (ctypes.c_int32 * (7 * len(rows)))(*[v for r in rows for v in r])
    f3 = (ctypes.c_float * 3)(1, 1, 1)
    p = ctypes.cast(f3, ctypes.c_void_p)
    return lib.dvt_frames_augment(64, frames, H0, W0, ctypes.cast(tab, ctypes.c_void_p), len(rows), 64, dst_dtype, out, out,
                                  p, p, 64, None)


def test_null_pointers_are_refused_by_name():
    lib = _lib()
    assert lib.dvt_frames_augment(None, 1, 4, 4, None, 1, None, 0, 2, 2, None, None, None, None) == -1
    assert b"dvt_frames_augment" in lib.dvt_last_error()
    assert lib.dvt_frames_erase(None, 0, 1, 4, 4, None, None, None) == -1
    assert b"dvt_frames_erase" in lib.dvt_last_error()


@pytest.mark.parametrize("row,what", [((0, 0, 0, 21, 4, 0, 0), b"leaves"), ((0, 17, 0, 4, 4, 0, 0), b"leaves"),
                                      ((0, 0, 27, 4, 4, 0, 0), b"leaves"), ((0, -1, 0, 4, 4, 0, 0), b"leaves"),
                                      ((0, 0, 0, 0, 4, 0, 0), b"leaves"), ((0, 0, 0, 4, 0, 0, 0), b"leaves"),
                                      ((2, 0, 0, 4, 4, 0, 0), b"src_index"), ((-1, 0, 0, 4, 4, 0, 0), b"src_index"),
                                      ((0, 0, 0, 4, 4, 2, 0), b"flips"), ((0, 0, 0, 4, 4, 0, -1), b"flips")])
def test_bad_augment_row_is_named(row, what):
    lib = _lib()
    good = (1, 16, 26, 4, 4, 1, 1)                                 # the last window that fits a 20 x 30 frame
    assert _augment(lib, [good, good, row, good]) == -1
    msg = lib.dvt_last_error()
    assert b"dvt_frames_augment" in msg and b"row 2" in msg and what in msg


def test_bad_erase_row_is_named():
    lib = _lib()
    f3 = ctypes.cast((ctypes.c_float * 3)(0, 0, 0), ctypes.c_void_p)
    for bad in ((0, 0, 9, 1), (8, 0, 1, 1), (0, 3, 1, 10), (0, 0, 2, 0), (-1, 0, 1, 1)):
        rows = [(0, 0, 0, 0), (7, 11, 1, 1), (5, 5, 0, -3), bad]   # h == 0: the other fields of the row are not read
        tab = (ctypes.c_int32 * 16)(*[v for r in rows for v in r])
        assert lib.dvt_frames_erase(64, 0, 4, 8, 12, ctypes.cast(tab, ctypes.c_void_p), f3, None) == -1
        msg = lib.dvt_last_error()
        assert b"dvt_frames_erase" in msg and b"row 3" in msg, (bad, msg)


def test_band_plan_and_refusal_without_a_gpu():
    """The workspace query is host arithmetic.  A geometry whose single output row needs more input rows than 64 KiB of
    LDS hold (4000 rows squeezed to 8, 1024 columns wide: 1001 rows of 3072 bytes) is refused by the query and, by name,
    by the launcher; the reference's largest (360 x 640 -> 224 x 224) is planned."""
    lib = _lib()
    assert lib.dvt_frames_augment_workspace_bytes(28, 360, 640, 224, 224) > 0
    assert lib.dvt_frames_augment_workspace_bytes(1, 600, 8, 16, 256) > 0          # fits with a band of one row
    assert lib.dvt_frames_augment_workspace_bytes(1, 4000, 8, 8, 1024) == 0
    tab = (ctypes.c_int32 * 7)(0, 0, 0, 4000, 8, 0, 0)
    p = ctypes.cast((ctypes.c_float * 3)(1, 1, 1), ctypes.c_void_p)
    rc = lib.dvt_frames_augment(64, 1, 4000, 8, ctypes.cast(tab, ctypes.c_void_p), 1, 64, 0, 8, 1024, p, p, 64, None)
    assert rc == -2 and b"dvt_frames_augment" in lib.dvt_last_error() and b"LDS" in lib.dvt_last_error()
