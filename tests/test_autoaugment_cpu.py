"""AutoAugment (the AutoAugment stage of MMX_Frame_dl.py:63-71) without a GPU: the numpy restatement (tests/autoaugment_ref.py)
against the fixture written through Pillow and against the installed Pillow, the host sampler of dvt_amd.input_stage, and the
C surface (declaration, enum, host-side validation of the table before any HIP call)."""
import ctypes
import importlib.util
import os
import re

import numpy as np
import pytest
import torch

from tests import autoaugment_ref as R
from tests.util import golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIZES = ("37x53", "48x64")
SIGNED_CASES = [f"{op}:{b}:{s}" for op in R.SIGNED for b, s in ((2, 0), (9, 1))]
CASES = SIGNED_CASES + [f"{op}:{b}:1" for op in ("Posterize", "Solarize") for b in (2, 9)] + [
    f"{op}:-1:1" for op in ("AutoContrast", "Equalize", "Invert")]


def case_slot(case: str, H: int, W: int):
    op, b, s = case.split(":")
    return R.slot(op, R.magnitude(op, int(b), int(s), H, W) if int(b) >= 0 else 0.0, H, W)


def _pillow():
    pytest.importorskip("PIL.Image")
    spec = importlib.util.spec_from_file_location("gen_golden_autoaugment", os.path.join(ROOT, "tools", "gen_golden_autoaugment.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


# ---------------------------------------------------------------- restatement
def test_fixture_holds_every_operation_at_two_bins_and_both_signs():
    g = golden("autoaugment.npz")
    assert tuple(g["cases"]) == tuple(CASES) and len(CASES) == 25
    ops = {c.split(":")[0] for c in CASES}
    assert ops == set(R.OPS) - {"Identity"} and len(ops) == 14
    for op in R.SIGNED + ("Posterize", "Solarize"):
        assert {c.split(":")[1] for c in CASES if c.startswith(op + ":")} == {"2", "9"}
    for op in R.SIGNED:
        assert {c.split(":")[2] for c in CASES if c.startswith(op + ":")} == {"0", "1"}


@pytest.mark.parametrize("size", SIZES)
@pytest.mark.parametrize("case", CASES)
def test_reference_matches_pillow_fixture(size, case):
    g = golden("autoaugment.npz")
    frame = g[size + ":frame"]
    H, W, _ = frame.shape
    assert f"{H}x{W}" == size
    u8 = R.apply_slot(frame, case_slot(case, H, W))
    assert u8.dtype == np.uint8 and np.array_equal(u8, g[f"{size}:{case}:u8"])
    if case.split(":")[0] not in R.GEOMETRIC:
        assert not np.array_equal(u8, frame)                      # the case does something
    f32 = R.normalize(u8[None], g["mean"], g["std"])[0]
    assert f32.dtype == np.float32 and np.array_equal(f32, g[f"{size}:{case}:f32"])


def _edge_images():
    rng = np.random.default_rng(5)
    out = {"random": rng.integers(0, 256, (37, 53, 3), dtype=np.uint8),
           "tiny": rng.integers(0, 256, (8, 8, 3), dtype=np.uint8),              # 64 pixels: Equalize has step == 0
           "dark": rng.integers(0, 30, (21, 30, 3), dtype=np.uint8),             # blends clip at 0 ...
           "bright": rng.integers(225, 256, (21, 30, 3), dtype=np.uint8),        # ... and at 255
           "skewed": (rng.integers(0, 256, (16, 20, 3)) ** 3 // 65536).astype(np.uint8)}   # Equalize: a small step
    const = rng.integers(0, 256, (21, 30, 3), dtype=np.uint8)
    const[..., 1] = 77                                                            # identity for Equalize and AutoContrast
    out["constant_channel"] = const
    return out


def test_reference_against_installed_pillow_every_bin_and_sign():
    G = _pillow()
    for name, img in _edge_images().items():
        H, W, _ = img.shape
        for op in R.OPS:
            for mid in range(10):
                for sign in (0, 1):
                    m = R.magnitude(op, mid, sign, H, W)
                    got = R.apply_slot(img, R.slot(op, m, H, W))
                    assert np.array_equal(got, G.pillow_u8(img, op, m)), (name, op, mid, sign)


def test_edge_inputs_take_the_branches_they_are_there_for():
    e = _edge_images()
    eq, ac = [R.OP_ID["Equalize"]] + [0] * 7, [R.OP_ID["AutoContrast"]] + [0] * 7
    assert np.array_equal(R.apply_slot(e["tiny"], eq), e["tiny"])                  # step == 0
    c = e["constant_channel"]
    assert np.array_equal(R.apply_slot(c, eq)[..., 1], c[..., 1]) and not np.array_equal(R.apply_slot(c, eq), c)
    assert np.array_equal(R.apply_slot(c, ac)[..., 1], c[..., 1])
    hi = R.apply_slot(e["bright"], R.slot("Brightness", 0.9, 21, 30))
    lo = R.apply_slot(e["dark"], R.slot("Contrast", 0.9, 21, 30))
    assert (hi == 255).all() and (lo == 0).any()


def test_reference_against_installed_pillow_all_sub_policies_both_ops_forced():
    G = _pillow()
    Image = pytest.importorskip("PIL.Image")
    rng = np.random.default_rng(9)
    for H, W in ((37, 53), (48, 64)):
        img = rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
        assert len(R.IMAGENET) == 25
        for sub in R.IMAGENET:
            for signs in ((0, 0), (1, 1), (0, 1)):
                pil = Image.fromarray(img)
                table = []
                for (op, _, mid), sign in zip(sub, signs):
                    m = R.magnitude(op, mid, sign, H, W)
                    pil = G.pillow_op(pil, op, m)
                    table.append(R.slot(op, m, H, W))
                got = R.apply_table(img[None], [table])[0]
                assert np.array_equal(got, np.asarray(pil)), (sub, signs)


# ---------------------------------------------------------------- the sampler
def _gen(seed):
    return torch.Generator().manual_seed(seed)


def test_policy_and_slots_match_the_restatement():
    from dvt_amd import input_stage as S
    assert S.IMAGENET_POLICY == R.IMAGENET and S.AUTOAUGMENT_OPS == R.OPS
    for H, W in ((37, 53), (224, 224)):
        for op in R.OPS:
            for mid in range(10):
                for sign in (0, 1):
                    m = S.autoaugment_magnitude(op, mid, sign, H, W)
                    assert m == R.magnitude(op, mid, sign, H, W)
                    assert S.autoaugment_slot(op, m, H, W) == R.slot(op, m, H, W), (op, mid, sign)
    # the documented bins
    assert S.autoaugment_magnitude("Rotate", 9, 1, 8, 8) == 30.0 and S.autoaugment_magnitude("Rotate", 9, 0, 8, 8) == -30.0
    assert S.autoaugment_magnitude("Solarize", 0, 0, 8, 8) == 255.0 and S.autoaugment_magnitude("Solarize", 9, 0, 8, 8) == 0.0
    assert [S.autoaugment_magnitude("Posterize", i, 0, 8, 8) for i in range(10)] == [8, 8, 7, 7, 6, 6, 5, 5, 4, 4]
    assert S.autoaugment_magnitude("TranslateX", 9, 1, 100, 331) == float(torch.tensor(150.0).item())
    assert S.autoaugment_slot("Posterize", 4.0, 8, 8)[:2] == [10, 0xF0]
    assert S.autoaugment_slot("Solarize", 56.66666793823242, 8, 8)[:2] == [11, 57]
    assert S.autoaugment_slot("TranslateY", -7.9, 8, 8) == [4, 65536, 0, 32768, 0, 65536, 32768 + 7 * 65536, 0]


def test_same_seed_same_table():
    from dvt_amd.input_stage import AutoAugment
    a = AutoAugment(generator=_gen(11)).draw(64, 37, 53)
    b = AutoAugment(generator=_gen(11)).draw(64, 37, 53)
    c = AutoAugment(generator=_gen(12)).draw(64, 37, 53)
    assert a.dtype == torch.int32 and a.shape == (64, 2, 8) and torch.equal(a, b) and not torch.equal(a, c)


def test_draw_order_is_policy_then_probabilities_then_signs():
    from dvt_amd.input_stage import AutoAugment
    H, W, n = 37, 53, 200
    table = AutoAugment(generator=_gen(3)).draw(n, H, W)
    g = _gen(3)
    seen = set()
    for row in table.tolist():
        policy_id = int(torch.randint(25, (1,), generator=g).item())
        probs = torch.rand((2,), generator=g)
        signs = torch.randint(2, (2,), generator=g)
        for i, entry in enumerate(R.IMAGENET[policy_id]):
            applied = bool(probs[i] <= entry[1])
            assert row[i] == (R.policy_slot(entry, int(signs[i]), H, W) if applied else [0] * 8)
            seen.add((entry[0], applied))
    assert {op for op, _ in seen} == {e[0] for sub in R.IMAGENET for e in sub}      # every operation of the policy was drawn
    assert any(not a for _, a in seen)


def test_probability_extremes_and_uniform_policy_index():
    from dvt_amd.input_stage import AutoAugment
    inv, sol = R.OP_ID["Invert"], R.OP_ID["Solarize"]
    t = AutoAugment(policy=[(("Invert", 1.0, None), ("Solarize", 0.0, 3))], generator=_gen(1)).draw(500, 20, 20)
    assert (t[:, 0, 0] == inv).all() and (t[:, 1, 0] == 0).all() and not t[:, 1].any()
    t = AutoAugment(policy=[(("Solarize", 1.0, 3), ("Invert", 0.0, None))], generator=_gen(1)).draw(500, 20, 20)
    assert (t[:, 0, 0] == sol).all() and (t[:, 0, 1] == R.slot("Solarize", R.magnitude("Solarize", 3, 0, 20, 20), 20, 20)[1]).all()
    assert not t[:, 1].any()
    # 25 sub-policies that name themselves, both operations always applied: sub-policy i has solarize bin i % 10 and
    # posterize bin 2 (i // 10), i.e. one of 10 thresholds and one of 3 masks
    n = 25000
    t = AutoAugment(policy=[(("Solarize", 1.0, i % 10), ("Posterize", 1.0, 2 * (i // 10))) for i in range(25)],
                    generator=_gen(2)).draw(n, 20, 20)
    thresholds = sorted({int(v) for v in t[:, 0, 1].tolist()}, reverse=True)
    masks = sorted({int(v) for v in t[:, 1, 1].tolist()}, reverse=True)
    assert len(thresholds) == 10 and len(masks) == 3
    index = torch.tensor([thresholds.index(int(a)) + 10 * masks.index(int(b)) for a, b in zip(t[:, 0, 1], t[:, 1, 1])])
    counts = torch.bincount(index, minlength=25)
    # binomial(25000, 1 / 25): mean 1000, sigma 31; six sigma
    assert counts.shape == (25,) and int(counts.min()) > 1000 - 186 and int(counts.max()) < 1000 + 186


def test_constructor_and_wrapper_refusals():
    from dvt_amd import ops
    from dvt_amd import input_stage as S
    with pytest.raises(NotImplementedError, match="cifar10"):
        S.AutoAugment("cifar10")
    with pytest.raises(ValueError, match="policy"):
        S.AutoAugment(policy=[(("Blur", 1.0, 1), ("Invert", 1.0, None))])
    with pytest.raises(ValueError, match="frames_u8"):
        S.AutoAugment()(torch.zeros(1, 20, 30, 3))
    u8 = torch.zeros(2, 20, 30, 3, dtype=torch.uint8)
    with pytest.raises(ValueError, match="frames_u8"):
        ops.frames_autoaugment(u8.float(), torch.zeros(2, 2, 8, dtype=torch.int32), (0, 0, 0), (1, 1, 1), torch.float32)
    with pytest.raises(ValueError, match="table"):
        ops.frames_autoaugment(u8, torch.zeros(3, 2, 8, dtype=torch.int32), (0, 0, 0), (1, 1, 1), torch.float32)
    with pytest.raises(ValueError, match="out_dtype"):
        ops.frames_autoaugment(u8, torch.zeros(2, 2, 8, dtype=torch.int32), (0, 0, 0), (1, 1, 1), torch.float64)
    with pytest.raises(ValueError, match="mean"):
        ops.frames_autoaugment(u8, torch.zeros(2, 2, 8, dtype=torch.int32), None, (1, 1, 1), torch.float32)
    t = S.train_transform_autoaugment(torch.float32)
    assert (t.first.size, t.first.hflip_p, t.first.vflip_p, t.first.dtype) == (224, 0.3, 0.3, torch.uint8)
    assert (t.second.policy, t.second.mean, t.second.std, t.second.dtype) == (S.IMAGENET_POLICY, S.IMAGENET_MEAN, S.IMAGENET_STD,
                                                                             torch.float32)
    with pytest.raises(NotImplementedError):                                       # unchanged: the new factory is the way in
        S.train_transform(torch.float32, auto_augment=True)


# ---------------------------------------------------------------- C surface
def _lib():
    import dvt_amd
    return dvt_amd._lib.load()


def test_header_declares_the_entry_point_and_the_enum():
    import dvt_amd
    header = open(os.path.join(ROOT, "include", "dvt_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", " ", header, flags=re.S)
    (params,) = re.findall(r"\bint\s+dvt_frames_autoaugment\s*\(([^()]*)\)\s*;", code)
    names = [p.split()[-1].lstrip("*") for p in params.split(",")]
    assert names == ["src", "samples", "H", "W", "table", "dst", "dst_dtype", "mean", "std", "stream"]
    res, args = dvt_amd._lib.SIGNATURES["dvt_frames_autoaugment"]
    assert res is ctypes.c_int and args == [ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_void_p,
                                            ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_void_p, ctypes.c_void_p]
    want = ("IDENTITY", "SHEAR_X", "SHEAR_Y", "TRANSLATE_X", "TRANSLATE_Y", "ROTATE", "BRIGHTNESS", "COLOR", "CONTRAST",
            "SHARPNESS", "POSTERIZE", "SOLARIZE", "AUTOCONTRAST", "EQUALIZE", "INVERT")
    assert dvt_amd._lib.ENUMS["dvt_autoaugment_op"] == {"DVT_AA_" + n: i for i, n in enumerate(want)}
    assert [n.replace("_", "").lower() for n in want] == [n.lower() for n in R.OPS]
    assert dvt_amd._lib.ENUMS["dvt_augment_dst"] == {"DVT_AUGMENT_U8_HWC": 8}      # not extended
    assert _lib().dvt_version() == 5 and dvt_amd._lib.ABI_VERSION == 5
    assert "[AutoAugment]" not in header and "MMX_Frame_dl.py:63-71" in header


def _call(lib, slots, H=20, W=30, src=64, dst=64, table=True, dst_dtype=0, mean=True, std=True):
    """dvt_frames_autoaugment on dummy non-null device pointers: everything is validated before anything touches them."""
    flat = [v for s in slots for v in s]
    tab = (ctypes.c_int32 * len(flat))(*flat)
    p = ctypes.cast((ctypes.c_float * 3)(1, 1, 1), ctypes.c_void_p)
    return lib.dvt_frames_autoaugment(src, len(slots) // 2, H, W, ctypes.cast(tab, ctypes.c_void_p) if table else None, dst,
                                      dst_dtype, p if mean else None, p if std else None, None)


IDENT = [0] * 8


@pytest.mark.parametrize("kw,name", [({"src": None}, b"src"), ({"dst": None}, b"dst"), ({"table": False}, b"table"),
                                     ({"mean": False}, b"mean"), ({"std": False}, b"std")])
def test_null_pointers_are_refused_by_name(kw, name):
    lib = _lib()
    assert _call(lib, [IDENT, IDENT], **kw) == -1
    msg = lib.dvt_last_error()
    assert b"dvt_frames_autoaugment" in msg and name + b" is null" in msg


@pytest.mark.parametrize("slot,what", [([15] + [0] * 7, b"op 15"), ([-1] + [0] * 7, b"op -1"),
                                       ([10, 0xF1] + [0] * 6, b"posterize mask 241"), ([10, 256] + [0] * 6, b"posterize mask"),
                                       ([10, 0x7F] + [0] * 6, b"posterize mask 127"), ([11, 257] + [0] * 6, b"solarize"),
                                       ([11, -1] + [0] * 6, b"solarize"), ([6, 0x7FC00000] + [0] * 6, b"blend factor"),
                                       ([9, 0x7F800000] + [0] * 6, b"blend factor")])
def test_bad_slot_is_named_before_any_hip_call(slot, what):
    lib = _lib()
    good = [10, 0xF0] + [0] * 6
    assert _call(lib, [good, IDENT, IDENT, good, good, slot]) == -1
    msg = lib.dvt_last_error()
    assert b"dvt_frames_autoaugment" in msg and b"sample 2 slot 1" in msg and what in msg, msg
    assert _call(lib, [slot, good]) == -1 and b"sample 0 slot 0" in lib.dvt_last_error()


def test_sizes_and_dtype_are_checked_on_the_host():
    lib = _lib()
    assert _call(lib, [IDENT, IDENT], H=2, W=30) == -1 and b"H, W >= 3" in lib.dvt_last_error()
    assert _call(lib, [IDENT, IDENT], dst_dtype=5) == -1 and b"dst_dtype 5" in lib.dvt_last_error()
    # 3 H W bytes must fit the LDS image: 231 x 231 = 160,083 bytes does not, and is refused as unsupported, by name
    assert _call(lib, [IDENT, IDENT], H=231, W=231) == -2
    assert b"dvt_frames_autoaugment" in lib.dvt_last_error() and b"LDS" in lib.dvt_last_error()
