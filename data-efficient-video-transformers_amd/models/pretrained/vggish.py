"""VGGish, the audio expert the reference names at ``src/models/pretrained/models.py:13`` (``torch.hub.load('harritaylor/
torchvggish', 'vggish')``, commented out there because torch.hub needs the network) and calls at ``:55-57``, on HIP kernels.

Neither torchvggish nor its checkpoint can be fetched here, so this module restates the public definition with the
checkpoint's state-dict keys (``features.{0,3,6,8,11,13}``, ``embeddings.{0,2,4}``); parity against torchvggish itself is
UNPINNED and is checked against a CPU restatement only (tests/audio_ref.py).

  waveform [..., L] (mono, 16 kHz, in [-1, 1]; decoding and resampling stay with the caller)
    -> ``examples``: log-mel examples [R * E, 96, 64], the NHWC map of a one-channel image (ops.logmel_examples)
    -> ``embed``: features (conv1 + pool fused in ops.vggish_conv1_pool; the other five convolutions on the inference
       implicit-GEMM route dvt_conv3d_implicit at T = 1, bias and ReLU in its epilogue; ops.maxpool_fwd at (2, 2, 0)), then three
       Linear + ReLU (ops.linear_fwd with the ReLU epilogue) -> [n, 128].

The PCA / 8-bit post-processor of the public model is not provided: ``postprocess=True`` raises, ``pproc.*`` keys of a
checkpoint are ignored.  Inference only.
"""
from __future__ import annotations

import sys

import torch
import torch.nn as nn

from ... import _lib as L
from ... import ops

__all__ = ["VGGish", "vggish", "SEED"]

# the convolutions behind conv1: (features index, Cin, Cout, H, W of its map, pool after it)
_CONVS = ((3, 64, 128, 48, 32, True), (6, 128, 256, 24, 16, False), (8, 256, 256, 24, 16, True), (11, 256, 512, 12, 8, False),
          (13, 512, 512, 12, 8, True))
_K3, _S1, _P1 = (1, 3, 3), (1, 1, 1), (0, 1, 1)          # a 3x3 / 1 / pad 1 convolution as dvt_conv3d_implicit states it (T = 1)
SEED = 4                                                  # of the seeded init (EmbeddingExtractor's audio_net uses it too)


def _make_features():
    layers, cin = [], 1
    for v in (64, "M", 128, "M", 256, 256, "M", 512, 512, "M"):
        if v == "M":
            layers.append(nn.MaxPool2d(kernel_size=2, stride=2))
        else:
            layers += [nn.Conv2d(cin, v, kernel_size=3, padding=1), nn.ReLU(inplace=True)]
            cin = v
    return nn.Sequential(*layers)


class VGGish(nn.Module):
    def __init__(self, *, compute_dtype: torch.dtype = torch.bfloat16, postprocess: bool = False):
        super().__init__()
        if postprocess:
            raise NotImplementedError("the PCA / 8-bit post-processor of the public VGGish is not provided: use the raw "
                                      "128-d embeddings (postprocess=False)")
        if compute_dtype not in (torch.bfloat16, torch.float16, torch.float32):
            raise ValueError(f"compute_dtype {compute_dtype}: expected bfloat16, float16 or float32")
        self.features = _make_features()
        self.embeddings = nn.Sequential(nn.Linear(512 * 4 * 6, 4096), nn.ReLU(True), nn.Linear(4096, 4096), nn.ReLU(True),
                                        nn.Linear(4096, 128), nn.ReLU(True))
        self.compute_dtype = compute_dtype
        for m in self.modules():                     # He-normal weights; small positive biases keep the ReLUs' outputs alive
            if isinstance(m, (nn.Conv2d, nn.Linear)):
                nn.init.kaiming_normal_(m.weight, mode="fan_in", nonlinearity="relu")
                nn.init.constant_(m.bias, 0.1)
        for p in self.parameters():
            p.requires_grad_(False)

    # ---------------------------------------------------------------- weights
    def load_state_dict(self, state_dict, strict: bool = True, **kw):
        """The public checkpoint's keys; the post-processor's (``pproc.*``) are ignored."""
        return super().load_state_dict({k: v for k, v in state_dict.items() if not k.startswith("pproc.")}, strict, **kw)

    def _packed(self, device):
        """Weights in the kernels' forms, made once and kept until a parameter changes or moves.  The route of the five
        convolutions is decided here and nowhere else: dvt_conv3d_implicit with T = 1, the one inference candidate that
        carries a per-channel shift (the bias) and the ReLU in its epilogue (ops.conv2d_implicit is the training route:
        bias-free, BatchNorm statistics behind it, so a bias + ReLU pass would have to follow it).  Its ``_k`` query is asked
        for each of the five fixed geometries; one it does not take raises there, with the library's message."""
        ps = list(self.parameters())
        stamp = (self.compute_dtype, str(device)) + tuple((p.data_ptr(), p._version) for p in ps)
        hit = self.__dict__.get("_dvt_pack")
        if hit is not None and hit[0] == stamp:
            return hit[1]
        dt = self.compute_dtype
        f32 = lambda t: t.detach().float().contiguous()      # noqa: E731
        pk = {"conv1": (f32(self.features[0].weight), f32(self.features[0].bias)), "convs": [], "fcs": []}
        for idx, cin, cout, H, W, _pool in _CONVS:
            conv = self.features[idx]
            w = conv.weight.detach().float().reshape(cout, cin, 1, 3, 3)
            K = ops.conv3d_implicit_k(torch.empty((0, cin), dtype=dt), (1, 1, H, W), cout, _K3, _S1, _P1)
            pk["convs"].append((ops.conv3d_weight_pack(w, cin, K, dt), f32(conv.bias)))
        for idx in (0, 2, 4):
            fc = self.embeddings[idx]
            w = f32(fc.weight)
            pk["fcs"].append((w if dt == torch.float32 else ops.cast(w, dt), f32(fc.bias)))
        self.__dict__["_dvt_pack"] = (stamp, pk)
        return pk

    # ---------------------------------------------------------------- forward
    def _check(self):
        if self.training:
            raise NotImplementedError("inference-only: VGGish is a feature extractor here (no training / backward path): "
                                      "call .eval() and run it under torch.no_grad()")

    def examples(self, waveform: torch.Tensor) -> torch.Tensor:
        """waveform [..., L] f32 on the device -> log-mel examples [R * E, 96, 64] in the compute dtype, R the product of the
        leading dims."""
        wave = waveform.reshape(-1, waveform.shape[-1])
        if wave.dtype != torch.float32:
            wave = ops.cast(wave, torch.float32)
        return ops.logmel_examples(wave, self.compute_dtype)

    def embed(self, examples: torch.Tensor) -> torch.Tensor:
        """examples [n, 96, 64] in the compute dtype -> [n, 128]."""
        self._check()
        if examples.dim() != 3 or tuple(examples.shape[1:]) != (ops.LOGMEL_FRAMES, ops.LOGMEL_BANDS):
            raise ValueError("VGGish.embed expects examples [n, 96, 64]")
        dt = self.compute_dtype
        if examples.dtype != dt:
            examples = ops.cast(examples, dt)
        n = examples.shape[0]
        if n == 0:
            return torch.empty((0, 128), dtype=dt, device=examples.device)
        pk = self._packed(examples.device)
        y = ops.vggish_conv1_pool(examples, *pk["conv1"])                      # NHWC [n * 48 * 32, 64]
        for (_idx, _cin, cout, H, W, pool), (w, b) in zip(_CONVS, pk["convs"]):
            y = ops.conv3d_implicit(y, w, (n, 1, H, W), cout, _K3, _S1, _P1, shift=b, relu=True)
            if pool:
                y, _ = ops.maxpool_fwd(y, n, cout, H, W, 2, 2, 0)
                H, W = H // 2, W // 2
        # The public model transposes NCHW -> NHWC before it flattens, so embeddings.0's columns are in (H, W, C) order: on
        # NHWC maps the flatten is this view, no transpose launch.
        y = y.view(n, H * W * 512)
        for w, b in pk["fcs"]:
            y = ops.linear_fwd(y, w, b, epilogue=L.EPI_RELU)
        return y

    def forward(self, waveform: torch.Tensor) -> torch.Tensor:
        """waveform [..., L] -> [..., E, 128]."""
        self._check()
        lead = tuple(waveform.shape[:-1])
        ex = self.examples(waveform)
        R = 1
        for s in lead:
            R *= s
        E = ex.shape[0] // R if R else ops.logmel_num_examples(waveform.shape[-1])
        return self.embed(ex).view(*lead, E, 128)


def vggish(weights=None, *, compute_dtype: torch.dtype = torch.bfloat16, postprocess: bool = False, seed: int = SEED) -> VGGish:
    """A VGGish with the state dict of the file ``weights`` (the public checkpoint's layout), or -- without a file -- a
    seeded random init and a one-line warning on stderr."""
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        net = VGGish(compute_dtype=compute_dtype, postprocess=postprocess)
    if weights:
        sd = torch.load(str(weights), map_location="cpu")
        if isinstance(sd, dict) and "state_dict" in sd and isinstance(sd["state_dict"], dict):
            sd = sd["state_dict"]
        net.load_state_dict(sd, strict=True)
    else:
        print(f"[VGGish] no weights file, seeded random init (seed {seed}) -- embeddings are not pretrained features",
              file=sys.stderr)
    return net.eval()
