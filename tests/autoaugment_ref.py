"""Numpy restatement of torchvision's ``AutoAugment`` on uint8 RGB images, as its PIL path computes it (the AutoAugment
stage of src/dataloaders/mmx/MMX_Frame_dl.py:63-71), for the tests.  TEST INFRASTRUCTURE: the device code is
csrc/autoaugment.hip and the host side dvt_amd/input_stage.py; nothing here is imported by the product.

Two layers, as in the C interface:
  ``magnitude`` / ``slot``   an operation name, magnitude bin and sign -> the magnitude torchvision would use -> the eight
                             int32 of a table slot {op, p0 .. p6} (affine matrices in Pillow's 16.16 fixed point, blend
                             factors as float32 bits, the posterize mask, the solarize threshold)
  ``apply_slot`` / ``apply_table``   a slot applied to an image [H, W, 3]; a table [n, 2, 8] applied to frames [n, H, W, 3]

tests/golden/autoaugment.npz (tools/gen_golden_autoaugment.py, through Pillow itself) pins every operation.
"""
from __future__ import annotations

import math

import numpy as np
import torch

OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness",
       "Posterize", "Solarize", "AutoContrast", "Equalize", "Invert")
OP_ID = {name: i for i, name in enumerate(OPS)}
GEOMETRIC = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")
BLEND = ("Brightness", "Color", "Contrast", "Sharpness")
SIGNED = GEOMETRIC + BLEND
POSTERIZE_BITS = (8, 8, 7, 7, 6, 6, 5, 5, 4, 4)
BINS = 10

# the ImageNet policy: 25 sub-policies of two (operation, probability, magnitude bin)
IMAGENET = (
    (("Posterize", 0.4, 8), ("Rotate", 0.6, 9)), (("Solarize", 0.6, 5), ("AutoContrast", 0.6, None)),
    (("Equalize", 0.8, None), ("Equalize", 0.6, None)), (("Posterize", 0.6, 7), ("Posterize", 0.6, 6)),
    (("Equalize", 0.4, None), ("Solarize", 0.2, 4)), (("Equalize", 0.4, None), ("Rotate", 0.8, 8)),
    (("Solarize", 0.6, 3), ("Equalize", 0.6, None)), (("Posterize", 0.8, 5), ("Equalize", 1.0, None)),
    (("Rotate", 0.2, 3), ("Solarize", 0.6, 8)), (("Equalize", 0.6, None), ("Posterize", 0.4, 6)),
    (("Rotate", 0.8, 8), ("Color", 0.4, 0)), (("Rotate", 0.4, 9), ("Equalize", 0.6, None)),
    (("Equalize", 0.0, None), ("Equalize", 0.8, None)), (("Invert", 0.6, None), ("Equalize", 1.0, None)),
    (("Color", 0.6, 4), ("Contrast", 1.0, 8)), (("Rotate", 0.8, 8), ("Color", 1.0, 2)),
    (("Color", 0.8, 8), ("Solarize", 0.8, 7)), (("Sharpness", 0.4, 7), ("Invert", 0.6, None)),
    (("ShearX", 0.6, 5), ("Equalize", 1.0, None)), (("Color", 0.4, 0), ("Equalize", 0.6, None)),
    (("Equalize", 0.4, None), ("Solarize", 0.2, 4)), (("Solarize", 0.6, 5), ("AutoContrast", 0.6, None)),
    (("Invert", 0.6, None), ("Equalize", 1.0, None)), (("Color", 0.6, 4), ("Contrast", 1.0, 8)),
    (("Equalize", 0.8, None), ("Equalize", 0.6, None)),
)


def magnitude(op: str, magnitude_id, sign: int, H: int, W: int) -> float:
    """The magnitude of bin ``magnitude_id``: float32 ``torch.linspace`` bins read back as Python floats, negated for a
    signed operation when ``sign == 0``.  Posterize: the number of bits.  Operations without a magnitude: 0.0."""
    if op == "Posterize":
        return float(POSTERIZE_BITS[magnitude_id])
    top = {"ShearX": 0.3, "ShearY": 0.3, "TranslateX": 150.0 / 331.0 * W, "TranslateY": 150.0 / 331.0 * H, "Rotate": 30.0,
           "Brightness": 0.9, "Color": 0.9, "Contrast": 0.9, "Sharpness": 0.9}
    if op == "Solarize":
        return float(torch.linspace(255.0, 0.0, BINS)[magnitude_id].item())
    if op not in top:
        return 0.0
    m = float(torch.linspace(0.0, top[op], BINS)[magnitude_id].item())
    return -m if sign == 0 else m


def _fix(v: float) -> int:
    return int(math.floor(v * 65536.0 + 0.5))


def affine_fixed(m) -> tuple:
    """Pillow's 16.16 coefficients (a0 .. a5) of the inverse affine matrix m; a2 and a5 carry the half-pixel offset."""
    return (_fix(m[0]), _fix(m[1]), _fix(m[2] + m[0] * 0.5 + m[1] * 0.5), _fix(m[3]), _fix(m[4]),
            _fix(m[5] + m[3] * 0.5 + m[4] * 0.5))


def rotate_matrix(angle: float, H: int, W: int) -> list:
    """``Image.rotate(angle)`` about the centre (w / 2, h / 2), without expansion."""
    r = -math.radians(angle % 360.0)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    cx, cy = W / 2, H / 2
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def inverse_matrix(op: str, mag: float, H: int, W: int) -> list:
    if op == "ShearX":
        return [1.0, mag, 0.0, 0.0, 1.0, 0.0]
    if op == "ShearY":
        return [1.0, 0.0, 0.0, mag, 1.0, 0.0]
    if op == "TranslateX":
        return [1.0, 0.0, -float(int(mag)), 0.0, 1.0, 0.0]
    if op == "TranslateY":
        return [1.0, 0.0, 0.0, 0.0, 1.0, -float(int(mag))]
    assert op == "Rotate"
    return rotate_matrix(mag, H, W)


def slot(op: str, mag: float, H: int, W: int) -> list:
    """{op, p0 .. p6} for an operation at magnitude ``mag`` on an H x W image."""
    p = [0] * 7
    if op in GEOMETRIC:
        p[:6] = affine_fixed(inverse_matrix(op, mag, H, W))
    elif op in BLEND:
        p[0] = int(np.float32(1.0 + mag).view(np.int32))
    elif op == "Posterize":
        p[0] = ~(2 ** (8 - int(mag)) - 1) & 0xFF
    elif op == "Solarize":
        p[0] = int(math.ceil(mag))
    return [OP_ID[op]] + p


def policy_slot(entry, sign: int, H: int, W: int) -> list:
    op, _, mid = entry
    return slot(op, magnitude(op, mid, sign, H, W), H, W)


# ---------------------------------------------------------------- the operations on one image, uint8 [H, W, 3]
def _affine(img, a):
    H, W, _ = img.shape
    a0, a1, a2, a3, a4, a5 = (int(v) for v in a)
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    xin = (a2 + a1 * y + a0 * x) >> 16
    yin = (a5 + a4 * y + a3 * x) >> 16
    inside = (xin >= 0) & (xin < W) & (yin >= 0) & (yin < H)
    out = np.zeros_like(img)
    out[inside] = img[yin[inside], xin[inside]]
    return out


def _luma(img):
    v = img.astype(np.int64)
    return ((19595 * v[..., 0] + 38470 * v[..., 1] + 7471 * v[..., 2] + 0x8000) >> 16).astype(np.uint8)


def _smooth(img):
    """``ImageFilter.SMOOTH``: float32 weights 1 / 13 and 5 / 13; the sum starts at 0.5 and takes the row below, the row
    itself and the row above in that order, each as ((left + centre) + right); the one-pixel border is copied."""
    k1, k5 = np.float32(1) / np.float32(13), np.float32(5) / np.float32(13)
    f = img.astype(np.float32)
    H, W, _ = img.shape
    out = img.copy()
    if H < 3 or W < 3:
        return out
    ss = np.full((H - 2, W - 2, 3), np.float32(0.5), np.float32)
    for dy, mid in ((2, k1), (1, k5), (0, k1)):
        r = f[dy: dy + H - 2]
        ss = ss + ((r[:, 0: W - 2] * k1 + r[:, 1: W - 1] * mid) + r[:, 2: W] * k1)
    c = np.where(ss <= 0, 0, np.where(ss >= 255, 255, np.trunc(ss)))
    out[1: H - 1, 1: W - 1] = c.astype(np.uint8)
    return out


def _blend(deg, img, f):
    f = np.float32(f)
    d = deg.astype(np.float32)
    v = d + f * (img.astype(np.float32) - d)
    assert v.dtype == np.float32
    if 0.0 <= f <= 1.0:
        return v.astype(np.int32).astype(np.uint8)               # truncation; the value lies in [0, 255]
    return np.where(v <= 0, 0, np.where(v >= 255, 255, np.trunc(v))).astype(np.uint8)


def _autocontrast_lut(ch):
    lo, hi = int(ch.min()), int(ch.max())
    if hi <= lo:
        return np.arange(256, dtype=np.uint8)
    scale = 255.0 / (hi - lo)
    offset = -lo * scale
    return np.array([min(255, max(0, int(i * scale + offset))) for i in range(256)], np.uint8)


def _equalize_lut(ch):
    h = np.bincount(ch.reshape(-1), minlength=256).astype(np.int64)
    nz = np.nonzero(h)[0]
    ident = np.arange(256, dtype=np.uint8)
    if len(nz) <= 1:
        return ident
    step = (int(h.sum()) - int(h[nz[-1]])) // 255
    if step == 0:
        return ident
    n = step // 2
    lut = []
    for i in range(256):
        lut.append(min(255, n // step))
        n += int(h[i])
    return np.array(lut, np.uint8)


def apply_slot(img: np.ndarray, s) -> np.ndarray:
    op, p = OPS[int(s[0])], [int(v) for v in s[1:]]
    if op == "Identity":
        return img.copy()
    if op in GEOMETRIC:
        return _affine(img, p[:6])
    if op in BLEND:
        f = np.array(p[0], np.int32).view(np.float32)
        if op == "Brightness":
            deg = np.zeros_like(img)
        elif op == "Color":
            deg = np.repeat(_luma(img)[..., None], 3, -1)
        elif op == "Contrast":
            L = _luma(img).astype(np.int64)
            deg = np.full_like(img, int(int(L.sum()) / L.size + 0.5))
        else:
            deg = _smooth(img)
        return _blend(deg, img, f)
    if op == "Posterize":
        return img & np.uint8(p[0])
    if op == "Solarize":
        return np.where(img.astype(np.int32) < p[0], img, 255 - img).astype(np.uint8)
    if op == "Invert":
        return 255 - img
    lut = _autocontrast_lut if op == "AutoContrast" else _equalize_lut
    return np.stack([lut(img[..., c])[img[..., c]] for c in range(3)], -1)


def apply_table(frames: np.ndarray, table) -> np.ndarray:
    """frames uint8 [n, H, W, 3], table [n, 2, 8] -> uint8 [n, H, W, 3]: the two slots of a sample in order."""
    table = np.asarray(table).reshape(len(frames), 2, 8)
    return np.stack([apply_slot(apply_slot(f, t[0]), t[1]) for f, t in zip(frames, table)])


def normalize(u8: np.ndarray, mean, std) -> np.ndarray:
    """uint8 [n, H, W, 3] -> float32 [n, 3, H, W]: ToTensor (/255) and Normalize, in float32 like torch."""
    mean32 = np.asarray(mean, np.float32).reshape(1, 3, 1, 1)
    std32 = np.asarray(std, np.float32).reshape(1, 3, 1, 1)
    return (u8.astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255) - mean32) / std32
