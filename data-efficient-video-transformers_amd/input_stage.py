"""On-device input stage: decoded uint8 frames -> normalised clip tensors.

Mirrors the ``transforms.Compose`` pipelines of the reference loaders for inputs that are already decoded RGB arrays in HBM:
the four deterministic ones (src/dataloaders/mmx/MMX_Light_dl.py:184-217) and the two random training ones of
src/dataloaders/mmx/MMX_Frame_dl.py -- ``RandomResizedCrop(224) -> flips -> [AutoAugment] -> ToTensor -> Normalize`` for every
training image (:63-71, live at :154) and ``Resize(120) -> CenterCrop(112) -> ToTensor -> Normalize -> RandomErasing()`` for
every training video frame (:81-88, live at :152-153).  MMX_Light_dl.py disables its image branch in ``__getitem__`` (:276);
MMX_Frame_dl.py, which feeds the ``frame`` / ``sum`` / ``distil`` / ``sum_residual`` / ``pre_modal`` modes, does not.

The random parameters are drawn on the host with the torch CPU generator, by torchvision's documented rules and in its
order (``RandomResizedCrop.get_params``, ``torch.rand(1) < p``, ``RandomErasing.get_params``); the kernels receive them as a
table.  AutoAugment's policy operations are not built: ``frames_augment(..., out_dtype=torch.uint8)`` is where they would go.
"""
from __future__ import annotations

import math

import torch

from . import ops

KINETICS_MEAN, KINETICS_STD = (0.43216, 0.394666, 0.37645), (0.22803, 0.22145, 0.216989)     # :206-207
IMAGENET_MEAN, IMAGENET_STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)                    # :191-192


class ClipPreprocessor:
    """``Resize(resize) -> CenterCrop(crop) -> ToTensor -> Normalize(mean, std)`` for whole batches of frames.

    ``__call__(frames)``: uint8 ``[..., H0, W0, 3]`` (any leading dims, e.g. ``[B, 13, 12, H0, W0, 3]``) ->
    ``[..., 3, crop, crop]`` in ``dtype`` -- the layout ``FrameTransformer.vid_step`` / ``ViViT.forward`` consume.
    """

    def __init__(self, resize: int, crop: int, mean=KINETICS_MEAN, std=KINETICS_STD, dtype: torch.dtype = torch.bfloat16):
        self.resize, self.crop, self.mean, self.std, self.dtype = resize, crop, tuple(mean), tuple(std), dtype

    def __call__(self, frames: torch.Tensor) -> torch.Tensor:
        lead = frames.shape[:-3]
        flat = frames.reshape(-1, *frames.shape[-3:])
        out = ops.frames_preprocess(flat, self.resize, self.crop, self.mean, self.std, self.dtype)
        return out.view(*lead, 3, self.crop, self.crop)


def train_vid(dtype=torch.bfloat16):      # MMX_Light_dl.py:203-208
    return ClipPreprocessor(120, 112, KINETICS_MEAN, KINETICS_STD, dtype)


def val_vid(dtype=torch.bfloat16):        # :211-217
    return ClipPreprocessor(112, 112, KINETICS_MEAN, KINETICS_STD, dtype)


def val_transform(dtype=torch.bfloat16):  # :195-201
    return ClipPreprocessor(230, 224, IMAGENET_MEAN, IMAGENET_STD, dtype)


def _uniform(lo: float, hi: float, generator) -> float:
    return torch.empty(1).uniform_(lo, hi, generator=generator).item()


def _randint(hi: int, generator) -> int:
    return int(torch.randint(0, hi, size=(1,), generator=generator).item())


def draw_resized_crop(H0: int, W0: int, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), generator=None):
    """``RandomResizedCrop.get_params``: (top, left, h, w) -- up to 10 tries of an area in ``scale`` and a log-uniform aspect
    in ``ratio``, then the central crop nearest to the ratio range."""
    area = H0 * W0
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        target_area = area * _uniform(scale[0], scale[1], generator)
        aspect = torch.exp(torch.empty(1).uniform_(float(log_ratio[0]), float(log_ratio[1]), generator=generator)).item()
        w = int(round(math.sqrt(target_area * aspect)))
        h = int(round(math.sqrt(target_area / aspect)))
        if 0 < w <= W0 and 0 < h <= H0:
            top = _randint(H0 - h + 1, generator)
            left = _randint(W0 - w + 1, generator)
            return top, left, h, w
    in_ratio = float(W0) / float(H0)
    if in_ratio < min(ratio):
        w = W0
        h = int(round(w / min(ratio)))
    elif in_ratio > max(ratio):
        h = H0
        w = int(round(h * max(ratio)))
    else:
        w, h = W0, H0
    return (H0 - h) // 2, (W0 - w) // 2, h, w


def draw_flip(p: float, generator=None) -> int:
    """``RandomHorizontalFlip`` / ``RandomVerticalFlip``: ``torch.rand(1) < p``."""
    return int(torch.rand(1, generator=generator).item() < p)


def draw_erase(H: int, W: int, p=0.5, scale=(0.02, 0.33), ratio=(0.3, 3.3), generator=None):
    """``RandomErasing.forward`` + ``get_params`` for one frame: (top, left, h, w), all zero when the frame is left alone
    (the coin, or 10 tries without ``h < H and w < W``)."""
    if not torch.rand(1, generator=generator).item() < p:
        return 0, 0, 0, 0
    area = H * W
    log_ratio = torch.log(torch.tensor(ratio))
    for _ in range(10):
        erase_area = area * _uniform(scale[0], scale[1], generator)
        aspect = torch.exp(torch.empty(1).uniform_(float(log_ratio[0]), float(log_ratio[1]), generator=generator)).item()
        h = int(round(math.sqrt(erase_area * aspect)))
        w = int(round(math.sqrt(erase_area / aspect)))
        if not (h < H and w < W):
            continue
        top = _randint(H - h + 1, generator)
        left = _randint(W - w + 1, generator)
        return (top, left, h, w) if h > 0 and w > 0 else (0, 0, 0, 0)
    return 0, 0, 0, 0


class RandomResizedCropFlip:
    """``RandomResizedCrop(size, scale, ratio) -> RandomHorizontalFlip(hflip_p) -> RandomVerticalFlip(vflip_p) -> ToTensor ->
    Normalize(mean, std)`` with one window and one pair of flips per sample.

    ``__call__(frames, index=None, params=None)``: uint8 ``[..., H0, W0, 3]`` -> ``[..., 3, size, size]`` in ``dtype``, one
    sample per frame.  ``index`` (a sequence of N positions among the flattened frames) -> ``[N, 3, size, size]``, sample n
    reading frame ``index[n]``: the loader's one random frame of a clip, or two views of one frame.  ``params``: a table
    ``[N, 7]`` (src_index, top, left, h, w, hflip, vflip) to use instead of drawing one; the table used is kept in
    ``.last_params`` (int32 CPU tensor), so that a saliency overlay can be mapped back to the frame.
    """

    def __init__(self, size: int, scale=(0.08, 1.0), ratio=(3.0 / 4.0, 4.0 / 3.0), hflip_p: float = 0.0, vflip_p: float = 0.0,
                 mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype: torch.dtype = torch.bfloat16, generator=None):
        self.size, self.scale, self.ratio = int(size), tuple(scale), tuple(ratio)
        self.hflip_p, self.vflip_p, self.mean, self.std, self.dtype = hflip_p, vflip_p, tuple(mean), tuple(std), dtype
        self.generator = generator
        self.last_params = None

    def draw(self, H0: int, W0: int, src_index) -> torch.Tensor:
        rows = []
        for i in src_index:
            top, left, h, w = draw_resized_crop(H0, W0, self.scale, self.ratio, self.generator)
            hf = draw_flip(self.hflip_p, self.generator)
            vf = draw_flip(self.vflip_p, self.generator)
            rows.append((int(i), top, left, h, w, hf, vf))
        return torch.tensor(rows, dtype=torch.int32).reshape(-1, 7)

    def __call__(self, frames: torch.Tensor, index=None, params=None) -> torch.Tensor:
        if not isinstance(frames, torch.Tensor) or frames.dtype != torch.uint8 or frames.dim() < 3 or frames.shape[-1] != 3:
            raise ValueError("frames must be uint8 [..., H0, W0, 3]")
        lead = frames.shape[:-3]
        flat = frames.reshape(-1, *frames.shape[-3:])
        H0, W0 = flat.shape[1], flat.shape[2]
        if params is None:
            params = self.draw(H0, W0, range(flat.shape[0]) if index is None else index)
        out = ops.frames_augment(flat, params, (self.size, self.size), self.mean, self.std, self.dtype)
        self.last_params = torch.as_tensor(params, dtype=torch.int32).clone()
        if index is None and out.shape[0] == flat.shape[0]:
            return out.view(*lead, 3, self.size, self.size)
        return out


class RandomErasing:
    """``transforms.RandomErasing(p, scale, ratio, value)`` on normalised frames, one rectangle drawn per frame (the reference
    applies the transform frame by frame).  ``__call__(x)``: ``[..., 3, H, W]`` contiguous, erased in place and returned; the
    table used (``[F, 4]``: top, left, h, w; h == 0 = untouched) is kept in ``.last_params``."""

    def __init__(self, p: float = 0.5, scale=(0.02, 0.33), ratio=(0.3, 3.3), value=0, generator=None):
        if isinstance(value, str):
            raise NotImplementedError("RandomErasing(value='random') is not built: only constant fills")
        self.p, self.scale, self.ratio, self.generator = p, tuple(scale), tuple(ratio), generator
        self.value = (float(value),) * 3 if isinstance(value, (int, float)) else tuple(float(v) for v in value)
        if len(self.value) != 3:
            raise ValueError("value must be a number or one number per channel")
        self.last_params = None

    def draw(self, H: int, W: int, frames: int) -> torch.Tensor:
        rows = [draw_erase(H, W, self.p, self.scale, self.ratio, self.generator) for _ in range(frames)]
        return torch.tensor(rows, dtype=torch.int32).reshape(-1, 4)

    def __call__(self, x: torch.Tensor, params=None) -> torch.Tensor:
        if not isinstance(x, torch.Tensor) or x.dim() < 3 or x.shape[-3] != 3:
            raise ValueError("x must be [..., 3, H, W]")
        flat = x.view(-1, *x.shape[-3:])
        if params is None:
            params = self.draw(flat.shape[2], flat.shape[3], flat.shape[0])
        ops.frames_erase(flat, params, self.value)
        self.last_params = torch.as_tensor(params, dtype=torch.int32).clone()
        return x


class _Then:
    """``second(first(frames))``: a preprocessor followed by an in-place stage."""

    def __init__(self, first, second):
        self.first, self.second = first, second

    def __call__(self, frames: torch.Tensor) -> torch.Tensor:
        return self.second(self.first(frames))


def train_transform(dtype=torch.bfloat16, auto_augment: bool = False, generator=None):      # MMX_Frame_dl.py:63-71
    if auto_augment:
        raise NotImplementedError("AutoAugment's policy operations are not built; they belong between the resample and "
                                  "ToTensor, on the uint8 output of ops.frames_augment(..., out_dtype=torch.uint8)")
    return RandomResizedCropFlip(224, hflip_p=0.3, vflip_p=0.3, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=dtype,
                                 generator=generator)


def train_vid_frame(dtype=torch.bfloat16, generator=None):                                  # MMX_Frame_dl.py:81-88
    return _Then(train_vid(dtype), RandomErasing(generator=generator))
