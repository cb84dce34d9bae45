"""Numpy restatement of the training augmentations of src/dataloaders/mmx/MMX_Frame_dl.py:63-71 and :81-88, for the tests.

Built from the unchanged ``oracle.input_stage.resize_bilinear_u8`` (Pillow's 8-bit bilinear resample, pinned against
Pillow by tests/golden/input_stage.npz): ``resized_crop`` is that resample applied to the SLICED window -- which is what
``img.crop(box).resize(size, BILINEAR)`` computes: the taps are clipped to the window, not to the frame, unlike
``img.resize(size, BILINEAR, box=box)`` -- followed by the two ``transpose`` flips, ToTensor and Normalize.
tests/golden/augment.npz (tools/gen_golden_augment.py, through Pillow itself) pins it.
"""
from __future__ import annotations

import numpy as np

from oracle.input_stage import resize_bilinear_u8


def augment_u8(frames: np.ndarray, table, out_h: int, out_w: int) -> np.ndarray:
    """frames uint8 [F, H0, W0, 3], table [N, 7] (src_index, top, left, h, w, hflip, vflip) -> uint8 [N, out_h, out_w, 3]."""
    table = np.asarray(table).reshape(-1, 7)
    out = np.empty((len(table), out_h, out_w, 3), np.uint8)
    for n, (f, top, left, h, w, hf, vf) in enumerate(table):
        img = resize_bilinear_u8(frames[f, top: top + h, left: left + w], out_h, out_w)
        if hf:
            img = img[:, ::-1]
        if vf:
            img = img[::-1]
        out[n] = img
    return out


def normalize(u8: np.ndarray, mean, std) -> np.ndarray:
    """uint8 [N, h, w, 3] -> float32 [N, 3, h, w]: ToTensor (/255) and Normalize, in float32 like torch."""
    mean32 = np.asarray(mean, np.float32).reshape(1, 3, 1, 1)
    std32 = np.asarray(std, np.float32).reshape(1, 3, 1, 1)
    t = u8.astype(np.float32).transpose(0, 3, 1, 2) / np.float32(255)
    return (t - mean32) / std32


def augment(frames: np.ndarray, table, out_h: int, out_w: int, mean, std) -> np.ndarray:
    return normalize(augment_u8(frames, table, out_h, out_w), mean, std)


def erase(x: np.ndarray, table, value=(0, 0, 0)) -> np.ndarray:
    """x [F, 3, H, W] -> a copy with x[f, c, top:top+h, left:left+w] = value[c] for every table row (top, left, h, w), h != 0."""
    out = x.copy()
    for f, (top, left, h, w) in enumerate(np.asarray(table).reshape(-1, 4)):
        if h:
            for c in range(3):
                out[f, c, top: top + h, left: left + w] = value[c]
    return out
