"""Mirror of the reference's ``src/models/pretrained/models.py``: ``EmbeddingExtractor``, the source of the expert features
that ``SimpleTransformer`` (``input_dimension: 2048``) and the MIT / MMX temporal loaders train on.

  image / location experts: ResNet-50 with ``fc = Identity()`` -> 2048-d per frame (``custom_resnet.ResNet.embed``, the 2-D
                            implicit-GEMM path), averaged over the frames;
  video expert:             r3d_18 with ``fc = Identity()`` -> 512-d per clip (``video_resnet.r3d_18``, one
                            ``dvt_conv3d_implicit`` launch per convolution).

Kept: the method names and return shapes (``init_models``, ``forward_img``, ``forward_location``, ``forward_video``,
``return_expert_for_key``, ``return_expert_for_key_pretrained``); the forward methods return CPU tensors.

Deviations: the reference downloads ImageNet / Kinetics weights; nothing is downloaded here.  The weights come from local
state-dict files in torchvision's key layout named by the optional config keys ``image_net_weights``, ``video_net_weights``
and ``location_net_weights`` (``fc.*`` keys are ignored); a net without a file gets a seeded random init and a one-line
warning on stderr.  ``compute_dtype`` (config, default bf16; "fp32" / "fp16" selectable).  The reference runs one forward
per image; here all of a key's frames go through one batched forward and the mean over the frames is taken on the device,
with one device-to-host copy at the end.  Depth expert: the reference never builds that network, its methods raise
``NotImplementedError``.  Audio expert: the reference names VGGish at models.py:13 (commented out: torch.hub) and calls it at
:55-57; it is built here only when the config carries ``audio_net: true`` or ``audio_net_weights: <path>`` (``vggish.VGGish``,
mono 16 kHz waveforms in, one 128-d vector per 0.96 s example out) -- without either key ``forward_audio`` raises
``NotImplementedError`` and ``return_expert_for_key("audio", ..)`` returns ``[]``, as before.
"""
from __future__ import annotations

import sys

import torch
import torch.nn as nn

from ... import functional as F
from ..custom_resnet import resnet50
from ..video_resnet import r3d_18
from .vggish import SEED as _AUDIO_SEED, vggish

__all__ = ["EmbeddingExtractor", "Identity"]

_DTYPES = {"bf16": torch.bfloat16, "bfloat16": torch.bfloat16, "fp16": torch.float16, "float16": torch.float16,
           "half": torch.float16, "fp32": torch.float32, "float32": torch.float32, "float": torch.float32}
_SEEDS = {"image_net": 0, "video_net": 1, "location_net": 2, "audio_net": _AUDIO_SEED}


class Identity(nn.Module):
    def forward(self, x):
        return x


def _cfg(config, key, default=None, typ=None):
    """config[key] from a dict or a confuse-style view (``config["gpu"].get(int)``); default when absent."""
    try:
        v = config[key]
    except (KeyError, IndexError, TypeError):
        return default
    if not isinstance(v, (dict, str, int, float, torch.dtype)) and v is not None and callable(getattr(v, "get", None)):
        try:
            v = v.get(typ) if typ is not None else v.get()
        except Exception as e:                   # confuse.NotFoundError (and friends) for a key that is not set
            if type(e).__name__ in ("NotFoundError", "KeyError", "ConfigError"):
                return default
            raise
    if v is None:
        return default
    return typ(v) if typ is not None and not isinstance(v, typ) else v


def _dtype(v) -> torch.dtype:
    if isinstance(v, torch.dtype):
        return v
    try:
        return _DTYPES[str(v).lower()]
    except KeyError:
        raise ValueError(f"compute_dtype {v!r}: expected one of {sorted(_DTYPES)}") from None


class EmbeddingExtractor:
    def __init__(self, config):
        gpu = _cfg(config, "gpu", 0, int)
        self.device = torch.device("cuda", gpu)
        self.compute_dtype = _dtype(_cfg(config, "compute_dtype", torch.bfloat16))
        self.image_net = self._build("image_net", resnet50, _cfg(config, "image_net_weights"))
        self.video_net = self._build("video_net", r3d_18, _cfg(config, "video_net_weights"))
        self.location_net = self._build("location_net", resnet50, _cfg(config, "location_net_weights"))
        self.audio_net = None
        audio_weights = _cfg(config, "audio_net_weights")
        if audio_weights or _cfg(config, "audio_net", False, bool):
            self.audio_net = vggish(audio_weights, compute_dtype=self.compute_dtype, seed=_SEEDS["audio_net"])

    def _build(self, name, factory, path):
        with torch.random.fork_rng(devices=[]):
            torch.manual_seed(_SEEDS[name])
            net = factory(compute_dtype=self.compute_dtype)
        net.fc = Identity()
        if path:
            sd = torch.load(str(path), map_location="cpu")
            if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
                sd = sd["state_dict"]
            sd = {k: v for k, v in sd.items() if not k.startswith("fc.")}
            net.load_state_dict(sd, strict=True)
        else:
            print(f"[EmbeddingExtractor] {name}: no {name}_weights file in the config, seeded random init "
                  f"(seed {_SEEDS[name]}) -- embeddings are not pretrained features", file=sys.stderr)
        return net

    def init_models(self, m):
        m = m.to(self.device)
        m = m.eval()
        return m

    # ---------------------------------------------------------------- device-resident batched forms
    def extract_images(self, frames, net=None):
        """frames [F, 3, H, W] -> [F, 2048] on the device (image expert; ``net``: another ResNet-50, e.g. location_net)."""
        net = self.init_models(self.image_net if net is None else net)
        with torch.no_grad():
            return net.embed(frames.to(self.device, non_blocking=True))

    def extract_video(self, clips):
        """clips [N, 3, T, H, W] -> [N, 512] on the device (video expert)."""
        net = self.init_models(self.video_net)
        with torch.no_grad():
            return net.features(clips.to(self.device, non_blocking=True))

    def extract_audio(self, waveform):
        """waveform [L] -> [E, 128]; [..., T, L] -> [..., T * E, 128] on the device (audio expert): one token per 0.96 s
        example, the E examples of each of the T chunks in order -- [B, 32, 16000] (32 one-second chunks) -> [B, 32, 128],
        the ``audio`` argument of PyramidViViT."""
        if self.audio_net is None:
            raise NotImplementedError("the audio expert (VGGish) is built only when the config carries audio_net: true or "
                                      "audio_net_weights: <path>")
        net = self.init_models(self.audio_net)
        with torch.no_grad():
            out = net(waveform.to(self.device, non_blocking=True))                # [..., E, 128]
        return out if waveform.dim() == 1 else out.flatten(-3, -2)

    def _mean_over_frames(self, raw, net):
        """raw: F images of [b, 1, 3, H, W] -> [b, 2048] = mean over the F images (the reference's stack -> transpose ->
        adaptive_avg_pool1d(1)), one batched forward of all b * F frames."""
        frames = torch.stack([img.squeeze(1) for img in raw], dim=1)            # [b, F, 3, H, W]
        b, nf = frames.shape[:2]
        emb = self.extract_images(frames.reshape(b * nf, *frames.shape[2:]), net)
        with torch.no_grad():
            out = F.mean_rows(emb.view(b, nf, emb.shape[1]))
        return out.cpu().float()

    # ---------------------------------------------------------------- the reference's surface
    def forward_img(self, tensor):
        return self.extract_images(tensor).cpu().float()

    def forward_location(self, tensor):
        return self.extract_images(tensor, self.location_net).cpu().float()

    def forward_video(self, tensor_stack):
        return self.extract_video(tensor_stack).cpu().float()

    def forward_depth(self, tensor):
        raise NotImplementedError("the depth expert (MiDaS) is never built by the reference (models.py:16); not provided")

    def forward_audio(self, audio_sample):
        return self.extract_audio(audio_sample).cpu().float()

    def depth_network_pool(self, depth_output):
        raise NotImplementedError("the depth expert (MiDaS) is never built by the reference; not provided")

    def return_expert_for_key(self, key, raw_tensor):
        if key == "image":
            return self._mean_over_frames(raw_tensor, self.image_net)
        if key == "motion" or key == "video":
            return self.forward_video(raw_tensor.unsqueeze(0))
        if key == "location":
            return self._mean_over_frames(raw_tensor, self.location_net)
        if key == "audio" and self.audio_net is not None:
            return self.forward_audio(raw_tensor)
        return []

    def return_expert_for_key_pretrained(self, key, raw_tensor):
        """Pre-extracted per-image embeddings -> the expert vector (host-side reshaping, as the reference does)."""
        output = []
        if key == "image" or key == "location":
            output = torch.stack(raw_tensor)
            output = output.transpose(0, 2)
            output = nn.functional.adaptive_avg_pool1d(output, 1)
            output = output.transpose(1, 0).squeeze(2)
            output = output.squeeze(1)
        if key == "motion" or key == "video":
            output = raw_tensor[0].unsqueeze(0)
        return output
