"""On-device input stage: decoded uint8 frames -> normalised clip tensors.

Mirrors the ``transforms.Compose`` pipelines of the reference loaders for inputs that are already decoded RGB arrays in HBM:
the four deterministic ones (src/dataloaders/mmx/MMX_Light_dl.py:184-217) and the two random training ones of
src/dataloaders/mmx/MMX_Frame_dl.py -- ``RandomResizedCrop(224) -> flips -> AutoAugment -> ToTensor -> Normalize`` for every
training image (:63-71, live at :154) and ``Resize(120) -> CenterCrop(112) -> ToTensor -> Normalize -> RandomErasing()`` for
every training video frame (:81-88, live at :152-153).  MMX_Light_dl.py disables its image branch in ``__getitem__`` (:276);
MMX_Frame_dl.py, which feeds the ``frame`` / ``sum`` / ``distil`` / ``sum_residual`` / ``pre_modal`` modes, does not.

The random parameters are drawn on the host with the torch CPU generator, by torchvision's documented rules and in its
order (``RandomResizedCrop.get_params``, ``torch.rand(1) < p``, ``RandomErasing.get_params``, ``AutoAugment.get_params``); the
kernels receive them as a table.  AutoAugment's operations run on the uint8 output of ``frames_augment(...,
out_dtype=torch.uint8)``: ``train_transform_autoaugment`` is the reference's whole line :63-71 (``train_transform`` is the line
without its AutoAugment stage).  The operations are Pillow's, as torchvision's PIL path calls them; their magnitudes, affine
matrices and 16.16 fixed-point coefficients are computed here on the host, so the kernel sees integers only.
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
    ``dtype=torch.uint8``: ``[..., size, size, 3]`` bytes, not normalised (the input of ``AutoAugment``).
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
            return out.view(*lead, *out.shape[1:])
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
    """The line without its AutoAugment stage; ``train_transform_autoaugment`` is the whole line."""
    if auto_augment:
        raise NotImplementedError("AutoAugment's policy operations are not built; they belong between the resample and "
                                  "ToTensor, on the uint8 output of ops.frames_augment(..., out_dtype=torch.uint8)")
    return RandomResizedCropFlip(224, hflip_p=0.3, vflip_p=0.3, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=dtype,
                                 generator=generator)


def train_vid_frame(dtype=torch.bfloat16, generator=None):                                  # MMX_Frame_dl.py:81-88
    return _Then(train_vid(dtype), RandomErasing(generator=generator))


# ---------------------------------------------------------------- AutoAugment (torchvision's, on its PIL path)
AUTOAUGMENT_OPS = ("Identity", "ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate", "Brightness", "Color", "Contrast",
                   "Sharpness", "Posterize", "Solarize", "AutoContrast", "Equalize", "Invert")      # = enum dvt_autoaugment_op
_AA_GEOMETRIC = ("ShearX", "ShearY", "TranslateX", "TranslateY", "Rotate")
_AA_BLEND = ("Brightness", "Color", "Contrast", "Sharpness")
_AA_BINS = 10
_AA_POSTERIZE_BITS = (8, 8, 7, 7, 6, 6, 5, 5, 4, 4)

# AutoAugmentPolicy.IMAGENET: 25 sub-policies of two (operation, probability, magnitude bin)
IMAGENET_POLICY = (
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


def autoaugment_magnitude(op: str, magnitude_id, sign: int, H: int, W: int) -> float:
    """``AutoAugment._augmentation_space(10, (H, W))``: bin ``magnitude_id`` of the operation's float32 ``torch.linspace``, as a
    Python float, negated for a signed operation when ``sign == 0``; Posterize: the number of bits; no magnitude: 0.0."""
    if op == "Posterize":
        return float(_AA_POSTERIZE_BITS[magnitude_id])
    if op == "Solarize":
        return float(torch.linspace(255.0, 0.0, _AA_BINS)[magnitude_id].item())
    if op in ("ShearX", "ShearY"):
        top = 0.3
    elif op == "TranslateX":
        top = 150.0 / 331.0 * W
    elif op == "TranslateY":
        top = 150.0 / 331.0 * H
    elif op == "Rotate":
        top = 30.0
    elif op in _AA_BLEND:
        top = 0.9
    else:
        return 0.0
    m = float(torch.linspace(0.0, top, _AA_BINS)[magnitude_id].item())
    return -m if sign == 0 else m


def _aa_inverse_matrix(op: str, mag: float, H: int, W: int):
    """The matrix Pillow's ``transform(AFFINE)`` receives: output pixel centre -> input position."""
    if op == "ShearX":                             # about the origin (F.affine(..., center=[0, 0])); torchvision passes
        # degrees(atan(mag)) and takes tan again: for all ten bins and both signs the 16.16 coefficient is the same
        return [1.0, mag, 0.0, 0.0, 1.0, 0.0]
    if op == "ShearY":
        return [1.0, 0.0, 0.0, mag, 1.0, 0.0]
    if op == "TranslateX":
        return [1.0, 0.0, -float(int(mag)), 0.0, 1.0, 0.0]
    if op == "TranslateY":
        return [1.0, 0.0, 0.0, 0.0, 1.0, -float(int(mag))]
    r = -math.radians(mag % 360.0)                 # Image.rotate about (W / 2, H / 2)
    m = [round(math.cos(r), 15), round(math.sin(r), 15), 0.0, round(-math.sin(r), 15), round(math.cos(r), 15), 0.0]
    cx, cy = W / 2, H / 2
    m[2] = m[0] * -cx + m[1] * -cy + m[2]
    m[5] = m[3] * -cx + m[4] * -cy + m[5]
    m[2] += cx
    m[5] += cy
    return m


def autoaugment_slot(op: str, mag: float, H: int, W: int):
    """The eight int32 {op, p0 .. p6} of a table slot of ``dvt_frames_autoaugment``: Pillow's 16.16 coefficients
    ``FIX(v) = floor(v * 65536 + 0.5)`` of a geometric operation (a2, a5 with the half-pixel offset), the float32 bits of a
    blend factor ``1 + mag``, the posterize mask, the solarize threshold ``ceil(mag)``."""
    p = [0] * 7
    if op in _AA_GEOMETRIC:
        m = _aa_inverse_matrix(op, mag, H, W)
        fix = lambda v: int(math.floor(v * 65536.0 + 0.5))  # noqa: E731
        p[:6] = [fix(m[0]), fix(m[1]), fix(m[2] + m[0] * 0.5 + m[1] * 0.5), fix(m[3]), fix(m[4]), fix(m[5] + m[3] * 0.5 + m[4] * 0.5)]
    elif op in _AA_BLEND:
        p[0] = int(torch.tensor(1.0 + mag, dtype=torch.float32).view(torch.int32).item())
    elif op == "Posterize":
        p[0] = ~(2 ** (8 - int(mag)) - 1) & 0xFF
    elif op == "Solarize":
        p[0] = int(math.ceil(mag))
    return [AUTOAUGMENT_OPS.index(op)] + p


class AutoAugment:
    """``transforms.AutoAugment(policy) -> ToTensor -> Normalize(mean, std)`` on uint8 frames, one sub-policy per sample.

    ``policy``: ``"imagenet"`` or a list of sub-policies ``((op, p, magnitude_id), (op, p, magnitude_id))`` with the names of
    ``AUTOAUGMENT_OPS``.  ``draw(n, H, W)`` makes torchvision's draws per sample, in its order -- ``randint(len(policy))``,
    ``rand(2)``, ``randint(2, (2,))`` -- and returns the int32 table ``[n, 2, 8]``; operation i applies when ``probs[i] <= p``,
    otherwise its slot is Identity.  ``__call__(frames_u8, params=None)``: uint8 ``[..., H, W, 3]`` -> ``[..., 3, H, W]`` in
    ``dtype`` (``torch.uint8``: ``[..., H, W, 3]``, not normalised); the table used is kept in ``.last_params``.
    """

    def __init__(self, policy="imagenet", mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype: torch.dtype = torch.bfloat16,
                 generator=None):
        if isinstance(policy, str):
            if policy != "imagenet":
                raise NotImplementedError(f"AutoAugment policy {policy!r} is not built: 'imagenet' or a list of sub-policies")
            policy = IMAGENET_POLICY
        self.policy = tuple(tuple((str(op), float(p), mid) for op, p, mid in sub) for sub in policy)
        for sub in self.policy:
            if len(sub) != 2 or any(op not in AUTOAUGMENT_OPS for op, _, _ in sub):
                raise ValueError(f"policy: a sub-policy is two (op, p, magnitude_id) with op in {AUTOAUGMENT_OPS}, got {sub}")
        self.mean, self.std, self.dtype, self.generator = tuple(mean), tuple(std), dtype, generator
        self.last_params = None

    def draw(self, n: int, H: int, W: int) -> torch.Tensor:
        rows = []
        for _ in range(n):
            policy_id = int(torch.randint(len(self.policy), (1,), generator=self.generator).item())
            probs = torch.rand((2,), generator=self.generator)
            signs = torch.randint(2, (2,), generator=self.generator)
            slots = []
            for i, (op, p, mid) in enumerate(self.policy[policy_id]):
                if probs[i] <= p:
                    slots.append(autoaugment_slot(op, autoaugment_magnitude(op, mid, int(signs[i]), H, W), H, W))
                else:
                    slots.append([0] * 8)
            rows.append(slots)
        return torch.tensor(rows, dtype=torch.int32).reshape(-1, 2, 8)

    def __call__(self, frames_u8: torch.Tensor, params=None) -> torch.Tensor:
        if (not isinstance(frames_u8, torch.Tensor) or frames_u8.dtype != torch.uint8 or frames_u8.dim() < 3
                or frames_u8.shape[-1] != 3):
            raise ValueError("frames_u8 must be uint8 [..., H, W, 3]")
        lead = frames_u8.shape[:-3]
        flat = frames_u8.reshape(-1, *frames_u8.shape[-3:])
        H, W = flat.shape[1], flat.shape[2]
        if params is None:
            params = self.draw(flat.shape[0], H, W)
        out = ops.frames_autoaugment(flat, params, self.mean, self.std, self.dtype)
        self.last_params = torch.as_tensor(params, dtype=torch.int32).reshape(-1, 2, 8).clone()
        return out.view(*lead, *out.shape[1:])


class _CropFlipAutoAugment:
    """``second(first(frames))`` with ``first`` a RandomResizedCropFlip writing uint8 and ``second`` an AutoAugment.
    ``__call__(frames, index=None, params=None, policy_params=None)`` as ``RandomResizedCropFlip.__call__``; the two tables
    used are ``.first.last_params`` and ``.second.last_params``, together ``.last_params``."""

    def __init__(self, first: RandomResizedCropFlip, second: AutoAugment):
        self.first, self.second = first, second
        self.last_params = None

    def __call__(self, frames: torch.Tensor, index=None, params=None, policy_params=None) -> torch.Tensor:
        u8 = self.first(frames, index=index, params=params)            # [..., size, size, 3] or [N, size, size, 3]
        out = self.second(u8, params=policy_params)
        self.last_params = (self.first.last_params, self.second.last_params)
        return out


def train_transform_autoaugment(dtype=torch.bfloat16, generator=None):                      # MMX_Frame_dl.py:63-71
    """The reference's whole training-image line: ``RandomResizedCrop(224) -> RandomHorizontalFlip(0.3) ->
    RandomVerticalFlip(0.3) -> AutoAugment() -> ToTensor -> Normalize``.  Crop and flips write uint8 through
    ``ops.frames_augment(..., out_dtype=torch.uint8)``; ``AutoAugment`` (ImageNet policy) reads that.  This factory, not
    ``train_transform(auto_augment=True)`` (which keeps refusing), is the way to the AutoAugment stage.  Accepts ``index=``
    as ``RandomResizedCropFlip`` does; one generator serves both stages, crop and flips of all samples drawn first."""
    first = RandomResizedCropFlip(224, hflip_p=0.3, vflip_p=0.3, mean=IMAGENET_MEAN, std=IMAGENET_STD, dtype=torch.uint8,
                                  generator=generator)
    return _CropFlipAutoAugment(first, AutoAugment("imagenet", IMAGENET_MEAN, IMAGENET_STD, dtype, generator))


# ---------------------------------------------------------------- Mixup / CutMix (timm.data.Mixup; VideoMix boxes for clips)
def draw_beta(alpha: float, generator=None, n=None):
    """``Beta(alpha, alpha)`` from the torch CPU generator: ``g1 / (g1 + g2)`` of two ``Gamma(alpha, 1)`` draws, an exact Beta
    sampler (``np.random.beta`` in timm).  A Python float, or with ``n`` a float64 tensor [n]."""
    g = torch._standard_gamma(torch.full((1 if n is None else int(n), 2), float(alpha), dtype=torch.float64),
                              generator=generator)
    lam = g[:, 0] / (g[:, 0] + g[:, 1])
    lam = torch.where(torch.isfinite(lam), lam, torch.full_like(lam, 0.5))       # both draws underflowed to 0
    return float(lam[0]) if n is None else lam


def _cut(size: int, ratio: float, generator):
    """timm's ``rand_bbox`` along one axis: a truncated integer side, a uniform integer centre, clipped to the axis."""
    side = int(size * ratio)
    centre = _randint(size, generator)
    return min(max(centre - side // 2, 0), size), min(max(centre + side // 2, 0), size)


def scale_box(row, src, dst):
    """The box ``(t0, t1, y0, y1, x0, x1)`` drawn on a ``src = (T, H, W)`` grid, on a ``dst`` grid: per axis
    ``lo' = lo * n' // n`` and ``hi' = ceil(hi * n' / n)`` -- the smallest box of the second grid that covers the first; an
    empty box stays empty and a full axis stays full."""
    out = []
    for a in range(3):
        lo, hi = int(row[2 * a]), int(row[2 * a + 1])
        n, m = int(src[a]), int(dst[a])
        out += [lo * m // n, lo * m // n] if hi <= lo else [lo * m // n, -((-hi * m) // n)]
    return out


class Mixup:
    """timm's ``Mixup`` for batches of clips: Mixup and CutMix across the batch with the partner ``B - 1 - i`` (the batch
    flip), and the mixed targets.  Arguments as timm's, plus ``generator`` (torch CPU generator of the draws) and ``box``:
    ``'tube'`` (VideoMix: a spatial box through every frame, side ratio ``sqrt(1 - lam)``), ``'spatiotemporal'`` (ratio
    ``cbrt(1 - lam)`` on t, y and x) or ``'temporal'`` (a run of ``int(T (1 - lam))`` whole frames).

    The draws follow timm's rule, on the host: ``rand < prob`` decides whether the batch (``mode='batch'``), the sample
    (``'elem'``) or the pair (``'pair'``, mirrored onto both members; the middle sample of an odd batch is left alone) is
    mixed; with both alphas positive ``rand < switch_prob`` picks CutMix; ``lam ~ Beta(alpha, alpha)``; a CutMix box has
    truncated integer sides, a uniform integer centre and is clipped to the clip, and its lambda is then corrected to
    ``1 - box volume / (T H W)``.  ``draw(B, T, H, W)`` -> ``(table, lam_input, lam_target)``: the int32 table [B, 8]
    (partner, kind, t0, t1, y0, y1, x0, x1; kind 0 = leave alone, 1 = mixup, 2 = cutmix) and two float32 [B].

    ``__call__(x, target, params=None)``: ``x`` is a tensor ``[B, ..., C, H, W]`` or a tuple of such tensors that share the
    batch and the table (FrameTransformer's ``img`` and ``vid``); they are mixed in place (``ops.clips_mix``) and returned.
    The box is drawn on the first tensor's ``(T, H, W)`` (T = the folded middle dimensions) and taken to another grid by
    ``scale_box``; ``lam_target`` is the first tensor's.  ``target``: float ``[B, C]`` (multi-label rows, mixed as they are,
    ``label_smoothing`` ignored) or int64 ``[B]`` (smoothed one-hot rows, needs ``num_classes``) -> float32 ``[B, C]`` from
    ``ops.targets_mix``.  ``params``: a ``draw`` result to use instead of drawing; what was used is kept in ``.last_params``.
    """

    def __init__(self, mixup_alpha=1.0, cutmix_alpha=0.0, cutmix_minmax=None, prob=1.0, switch_prob=0.5, mode="batch",
                 label_smoothing=0.1, num_classes=None, generator=None, box="tube"):
        if cutmix_minmax is not None:
            raise NotImplementedError("Mixup(cutmix_minmax=) is not built: boxes come from the Beta draw")
        if mode not in ("batch", "elem", "pair"):
            raise ValueError(f"mode must be 'batch', 'elem' or 'pair', got {mode!r}")
        if box not in ("tube", "spatiotemporal", "temporal"):
            raise ValueError(f"box must be 'tube', 'spatiotemporal' or 'temporal', got {box!r}")
        self.mixup_alpha, self.cutmix_alpha, self.prob, self.switch_prob = float(mixup_alpha), float(cutmix_alpha), prob, switch_prob
        self.mode, self.label_smoothing, self.num_classes, self.generator, self.box = mode, float(label_smoothing), num_classes, generator, box
        self.last_params = None

    def _draw_one(self, T: int, H: int, W: int):
        """-> (kind, t0, t1, y0, y1, x0, x1, lam_input, lam_target) of one batch, sample or pair"""
        g = self.generator
        leave = (0, 0, 0, 0, 0, 0, 0, 1.0, 1.0)
        if not (self.prob and (self.mixup_alpha > 0 or self.cutmix_alpha > 0)) or not torch.rand(1, generator=g).item() < self.prob:
            return leave
        if self.mixup_alpha > 0 and self.cutmix_alpha > 0:
            cut = torch.rand(1, generator=g).item() < self.switch_prob
        else:
            cut = self.cutmix_alpha > 0
        lam = draw_beta(self.cutmix_alpha if cut else self.mixup_alpha, g)
        if lam == 1.0:
            return leave
        if not cut:
            lam32 = float(torch.tensor(lam, dtype=torch.float32))
            return (1, 0, T, 0, H, 0, W, lam32, lam32)
        t0, t1, y0, y1, x0, x1 = 0, T, 0, H, 0, W
        if self.box == "tube":
            r = math.sqrt(1.0 - lam)
            (y0, y1), (x0, x1) = _cut(H, r, g), _cut(W, r, g)
        elif self.box == "spatiotemporal":
            r = (1.0 - lam) ** (1.0 / 3.0)
            (t0, t1), (y0, y1), (x0, x1) = _cut(T, r, g), _cut(H, r, g), _cut(W, r, g)
        else:
            t0, t1 = _cut(T, 1.0 - lam, g)
        lam_t = 1.0 - ((t1 - t0) * (y1 - y0) * (x1 - x0)) / float(T * H * W)
        return (2, t0, t1, y0, y1, x0, x1, lam_t, lam_t)

    def draw(self, B: int, T: int, H: int, W: int):
        if self.mode == "batch":
            rows = [self._draw_one(T, H, W)] * B
        elif self.mode == "elem":
            rows = [self._draw_one(T, H, W) for _ in range(B)]
        else:
            half = [self._draw_one(T, H, W) for _ in range(B // 2)]
            rows = half + ([(0, 0, 0, 0, 0, 0, 0, 1.0, 1.0)] if B % 2 else []) + half[::-1]
        table = torch.tensor([[B - 1 - i, *r[:7]] for i, r in enumerate(rows)], dtype=torch.int32).reshape(-1, 8)
        lam_input = torch.tensor([r[7] for r in rows], dtype=torch.float32)
        lam_target = torch.tensor([r[8] for r in rows], dtype=torch.float32)
        return table, lam_input, lam_target

    @staticmethod
    def _grid(t: torch.Tensor):
        if not isinstance(t, torch.Tensor) or t.dim() < 4:
            raise ValueError("x must be [B, ..., C, H, W] (or a tuple of such tensors)")
        C, H, W = t.shape[-3:]
        return (int(t[0].numel() // (C * H * W)) if t.shape[0] else 1, H, W)

    def __call__(self, x, target, params=None):
        xs = tuple(x) if isinstance(x, (tuple, list)) else (x,)
        grids = [self._grid(t) for t in xs]
        B = xs[0].shape[0]
        if any(t.shape[0] != B for t in xs) or target.shape[0] != B:
            raise ValueError("x (every tensor of it) and target share the batch dimension")
        soft = target.is_floating_point()
        if not soft and (target.dtype != torch.int64 or target.dim() != 1):
            raise ValueError("target must be float [B, C] or int64 [B]")
        if not soft and self.num_classes is None:
            raise ValueError("Mixup: int64 labels need num_classes")
        table, lam_input, lam_target = self.draw(B, *grids[0]) if params is None else params
        table = torch.as_tensor(table, dtype=torch.int32).reshape(-1, 8)
        for t, grid in zip(xs, grids):
            tab = table
            if grid != grids[0]:
                tab = table.clone()
                for i in range(B):
                    tab[i, 2:] = torch.tensor(scale_box(table[i, 2:].tolist(), grids[0], grid), dtype=torch.int32)
            ops.clips_mix(t, tab, lam_input)
        if soft:
            mixed = ops.targets_mix(table, lam_target, y=target.float())
        else:
            mixed = ops.targets_mix(table, lam_target, labels=target, num_classes=self.num_classes,
                                    smoothing=self.label_smoothing)
        self.last_params = (table.clone(), torch.as_tensor(lam_input, dtype=torch.float32).clone(),
                            torch.as_tensor(lam_target, dtype=torch.float32).clone())
        return x, mixed
