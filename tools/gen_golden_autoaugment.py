#!/usr/bin/env python3
"""Write tests/golden/autoaugment.npz: every AutoAugment operation (the AutoAugment stage of MMX_Frame_dl.py:63-71) THROUGH
PILLOW ITSELF -- the calls torchvision's PIL path makes (``Image.transform(AFFINE, NEAREST)``, ``Image.rotate``,
``ImageEnhance.*``, ``ImageOps.*``) -- with ToTensor / Normalize restated in float32 (torchvision is not installed).

One frame per size; single operations only.  Every operation is stored at a low and a high magnitude bin, a signed one
negative at the low bin and positive at the high one (both signs, and for the blends both the truncating range f < 1 and the
clipping range f > 1), operations without a magnitude once: 25 cases per size, to keep the file small.  Stored per case:
the uint8 result [H, W, 3] and the float32 normalised result [3, H, W]; per size the frame; once the list of cases
``op:bin:sign``.  The magnitudes are torchvision's bins (float32 ``torch.linspace``), computed here and not taken from the
code under test.

    python tools/gen_golden_autoaugment.py
"""
from __future__ import annotations

import math
import os

import numpy as np
import torch
from PIL import Image, ImageEnhance, ImageOps

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "autoaugment.npz")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SIZES = ((37, 53), (48, 64))
LOW, HIGH = 2, 9
SIGNED = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast", "Sharpness")
UNSIGNED = ("Posterize", "Solarize")
PLAIN = ("AutoContrast", "Equalize", "Invert")
POSTERIZE_BITS = (8, 8, 7, 7, 6, 6, 5, 5, 4, 4)


def bin_magnitude(op: str, magnitude_id: int, sign: int, H: int, W: int) -> float:
    """torchvision's ``_augmentation_space(10, (H, W))`` bin, negated for a signed operation when ``sign == 0``."""
    if op == "Posterize":
        return float(POSTERIZE_BITS[magnitude_id])
    if op == "Solarize":
        return float(torch.linspace(255.0, 0.0, 10)[magnitude_id].item())
    top = {"ShearX": 0.3, "ShearY": 0.3, "TranslateX": 150.0 / 331.0 * W, "TranslateY": 150.0 / 331.0 * H, "Rotate": 30.0}
    m = float(torch.linspace(0.0, top.get(op, 0.9), 10)[magnitude_id].item())
    return m if sign else -m


def pillow_op(img: Image.Image, op: str, magnitude: float) -> Image.Image:
    """torchvision's ``_apply_op`` on a PIL image: nearest interpolation, black fill, shear about the origin."""
    affine = {"ShearX": (1, magnitude, 0, 0, 1, 0), "ShearY": (1, 0, 0, magnitude, 1, 0),
              "TranslateX": (1, 0, -int(magnitude), 0, 1, 0), "TranslateY": (1, 0, 0, 0, 1, -int(magnitude))}
    if op in affine:
        return img.transform(img.size, Image.AFFINE, affine[op], Image.NEAREST, fillcolor=(0, 0, 0))
    if op == "Rotate":
        return img.rotate(magnitude, Image.NEAREST, expand=False, fillcolor=(0, 0, 0))
    if op in ("Brightness", "Color", "Contrast", "Sharpness"):
        return getattr(ImageEnhance, op)(img).enhance(1.0 + magnitude)
    if op == "Posterize":
        return ImageOps.posterize(img, int(magnitude))
    if op == "Solarize":
        return ImageOps.solarize(img, magnitude)
    if op == "AutoContrast":
        return ImageOps.autocontrast(img)
    if op == "Equalize":
        return ImageOps.equalize(img)
    if op == "Invert":
        return ImageOps.invert(img)
    if op == "Identity":
        return img.copy()
    raise ValueError(op)


def pillow_u8(frame: np.ndarray, op: str, magnitude: float) -> np.ndarray:
    return np.asarray(pillow_op(Image.fromarray(frame), op, magnitude)).copy()


def cases():
    """(op, magnitude bin or -1, sign) of every stored case."""
    out = [(op, b, s) for op in SIGNED for b, s in ((LOW, 0), (HIGH, 1))]
    out += [(op, b, 1) for op in UNSIGNED for b in (LOW, HIGH)]
    return out + [(op, -1, 1) for op in PLAIN]


def test_frame(rng, H: int, W: int) -> np.ndarray:
    """A frame whose channels differ in range and histogram: a ramp with noise (most bins used, unevenly), a narrow band
    (AutoContrast has work to do) and a channel that reaches 0 and 255 (blends clip at both ends)."""
    yy, xx = np.mgrid[0:H, 0:W]
    r = np.clip(yy * 231 // (H - 1) + rng.integers(0, 24, (H, W)), 0, 255)
    g = 60 + (xx * 90 // (W - 1) + rng.integers(0, 12, (H, W)))
    b = np.where((yy // 6 + xx // 6) % 2 == 0, rng.integers(0, 16, (H, W)), 255 - rng.integers(0, 16, (H, W)))
    b[0, 0], b[-1, -1] = 0, 255
    return np.stack([r, g, b], -1).astype(np.uint8)


def main():
    rng = np.random.default_rng(1130 + 59)
    out = {"mean": np.array(MEAN), "std": np.array(STD)}
    mean32 = np.asarray(MEAN, np.float32).reshape(3, 1, 1)
    std32 = np.asarray(STD, np.float32).reshape(3, 1, 1)
    names = [f"{op}:{b}:{s}" for op, b, s in cases()]
    out["cases"] = np.array(names)
    for H, W in SIZES:
        frame = test_frame(rng, H, W)
        out[f"{H}x{W}:frame"] = frame
        for name, (op, b, s) in zip(names, cases()):
            m = bin_magnitude(op, b, s, H, W) if b >= 0 else 0.0
            u8 = pillow_u8(frame, op, m)
            assert not math.isnan(m) and u8.shape == frame.shape
            out[f"{H}x{W}:{name}:u8"] = u8
            out[f"{H}x{W}:{name}:f32"] = (u8.astype(np.float32).transpose(2, 0, 1) / np.float32(255) - mean32) / std32
    np.savez_compressed(OUT, **out)
    print("autoaugment:", len(names), "cases x", SIZES, "->", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
