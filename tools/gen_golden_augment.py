#!/usr/bin/env python3
"""Write tests/golden/augment.npz: the resample cases of the training augmentations (MMX_Frame_dl.py:63-71) THROUGH PILLOW
ITSELF -- ``Image.crop`` -> ``Image.resize(BILINEAR)`` -> ``Image.transpose`` -- with ToTensor / Normalize restated in
float32 (torchvision is not installed).  Stored per case: frames, the table, the expected uint8 [N, h, w, 3] and the
expected float32 [N, 3, h, w].  Every window is stored with all four flip combinations.

    python tools/gen_golden_augment.py
"""
from __future__ import annotations

import os

import numpy as np
from PIL import Image

OUT = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests", "golden", "augment.npz")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)
SIZES = ((37, 53), (48, 64))
# tag -> (out_h, out_w) or None (= the window's own size), window(H0, W0) -> (top, left, h, w)
CASES = {
    "whole": ((24, 24), lambda H, W: (0, 0, H, W)),
    "pixel_first": ((24, 24), lambda H, W: (0, 0, 1, 1)),
    "pixel_last": ((24, 24), lambda H, W: (H - 1, W - 1, 1, 1)),
    "interior_up": ((24, 24), lambda H, W: (5, 7, 9, 11)),
    "wide_down": ((8, 8), lambda H, W: (3, 0, 34, W)),             # full width: 53 / 8 -> 15 taps, 64 / 8 -> 17
    "tall_right": ((40, 40), lambda H, W: (0, W - 13, 37, 13)),    # touches the right edge
    "down_up": ((17, 17), lambda H, W: (10, 10, 5, 30)),
    "identity": (None, lambda H, W: (4, 6, 19, 21)),
}


def pillow_case(frame: np.ndarray, top, left, h, w, hf, vf, out_h, out_w) -> np.ndarray:
    img = Image.fromarray(frame).crop((left, top, left + w, top + h)).resize((out_w, out_h), Image.BILINEAR)
    if hf:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    if vf:
        img = img.transpose(Image.FLIP_TOP_BOTTOM)
    return np.asarray(img).copy()


def main():
    rng = np.random.default_rng(1130 + 41)
    out = {"mean": np.array(MEAN), "std": np.array(STD), "tags": np.array(list(CASES))}
    mean32 = np.asarray(MEAN, np.float32).reshape(1, 3, 1, 1)
    std32 = np.asarray(STD, np.float32).reshape(1, 3, 1, 1)
    for H0, W0 in SIZES:
        frames = rng.integers(0, 256, (3, H0, W0, 3), dtype=np.uint8)
        yy, xx = np.mgrid[0:H0, 0:W0]
        frames[0] = np.stack([yy * 255 // (H0 - 1), xx * 255 // (W0 - 1), (yy + xx) % 256], -1).astype(np.uint8)
        out[f"{H0}x{W0}:frames"] = frames
        for tag, (size, window) in CASES.items():
            top, left, h, w = window(H0, W0)
            out_h, out_w = size or (h, w)
            table, exp = [], []
            for i, (hf, vf) in enumerate(((0, 0), (1, 0), (0, 1), (1, 1))):
                f = i % 3
                table.append((f, top, left, h, w, hf, vf))
                exp.append(pillow_case(frames[f], top, left, h, w, hf, vf, out_h, out_w))
            u8 = np.stack(exp)
            key = f"{H0}x{W0}:{tag}"
            out[key + ":table"] = np.array(table, np.int32)
            out[key + ":size"] = np.array([out_h, out_w])
            out[key + ":u8"] = u8
            out[key + ":f32"] = (u8.astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255) - mean32) / std32
    np.savez_compressed(OUT, **out)
    print("augment:", list(CASES), "x", SIZES, "->", os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
