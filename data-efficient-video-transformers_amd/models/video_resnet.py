"""R(2+1)D-18 video backbone (``torchvision.models.video.r2plus1d_18``, used by the reference's
``VidResNet``, src/models/frame_transformer.py:64-74) on HIP kernels.  SURVEY section 8 row a11.

torchvision is not installed in the build image and its pretrained weights need the network, so
this module restates the public architecture (same module tree => same state-dict keys:
``stem.{0,1,3,4}``, ``layer{1..4}.{i}.conv{1,2}.0.{0,1,3}``, ``...conv{1,2}.1``,
``...downsample.{0,1}``, ``fc``); parity against torchvision itself is UNPINNED (no golden vectors
can be produced here) and is checked against a torch-CPU conv3d restatement only.

Layout: activations are NDHWC matrices [(n t h w), C].  The factorised convolutions map onto the
2-D path: (1,k,k) spatial = a 2-D conv over the N*T frames; (3,1,1) temporal = a (3,1) conv over
the [T, H*W] view of each clip; the strided 1x1x1 downsample = two strided row gathers + a GEMM.
"""
from __future__ import annotations

import torch
import torch.nn as nn

from .. import functional as F
from .. import ops


class Conv2Plus1D(nn.Sequential):
    def __init__(self, in_planes, out_planes, midplanes, stride=1, padding=1):
        super().__init__(
            nn.Conv3d(in_planes, midplanes, kernel_size=(1, 3, 3), stride=(1, stride, stride),
                      padding=(0, padding, padding), bias=False),
            nn.BatchNorm3d(midplanes),
            nn.ReLU(inplace=True),
            nn.Conv3d(midplanes, out_planes, kernel_size=(3, 1, 1), stride=(stride, 1, 1),
                      padding=(padding, 0, 0), bias=False),
        )

    @staticmethod
    def get_downsample_stride(stride):
        return stride, stride, stride


CPAD = 64     # mid-plane counts 45 / 230 / 460 / 921 are zero-padded to multiples of 64 (MFMA / LDS-DMA tile widths)


def _mid_cpad(conv, frames, H, W, dtype):
    """Channel padding of a spatial convolution's mid planes.  Multiples of 32 (288, 576, 1152) are whole k-tiles per filter
    tap for every consumer as they are; layer 1's 144 stay 144 where the streamed-weight halo kernels take the layer and its
    data gradient (ops.conv3x3_stream: the temporal convolution behind reads 144-channel pixels through the implicit
    kernels' per-lane taps) -- 192 would be a third more bytes and MFMA work on every mid-plane map; the rest is padded to
    the 64-wide tiles."""
    c = conv.out_channels
    if dtype not in (torch.bfloat16, torch.float16):
        return CPAD
    if c % 32 == 0:
        return 32
    if (c == 144 and conv.in_channels == 64 and F.is_3x3_same(conv.kernel_size[1:], conv.stride[1:], conv.padding[1:])
            and ops.conv3x3_stream_geometry(frames, H, W, 144, 64, dtype) and ops.conv3x3_stream_geometry(frames, H, W, 64, 144, dtype)):
        return 16
    return CPAD


def _spatial(fm, conv, bn, relu, dtype, fork=None, defer=False):
    """(1,k,k) conv + BN(+ReLU) on an NDHWC matrix: 2-D conv over N*T frames.  fork="alias": the map has a second consumer
    (the block's shortcut); the layer hands it out as a second result so that the shortcut's gradient joins this layer's
    data gradient inside the kernel that writes it (F._ConvBnAct) -> (fm, alias).  defer: the BatchNorm (+ ReLU) is NOT
    applied here -- the map returned is the convolution's output z and the third result the affine the temporal half behind
    applies inside its window kernels (see _virtual_bn_pair) -> (fm, alias or None, affine)."""
    y, N, T, H, W = fm
    k, s, p = conv.kernel_size[1:], conv.stride[1:], conv.padding[1:]
    Ho, Wo = (H + 2 * p[0] - k[0]) // s[0] + 1, (W + 2 * p[1] - k[1]) // s[1] + 1
    cpad = _mid_cpad(conv, N * T, H, W, dtype)
    if defer:
        out, affine = F.conv_bn_act_raw(y, conv.weight, bn, (N * T, y.shape[1], H, W, False), k, s, p, relu=relu, dtype=dtype,
                                        cpad=cpad, fork=fork, defer_apply=True)
        if fork is not None:
            return (out[0], N, T, Ho, Wo), out[1], affine
        return (out, N, T, Ho, Wo), None, affine
    out = F.conv_bn_act_raw(y, conv.weight, bn, (N * T, y.shape[1], H, W, False), k, s, p, relu=relu, dtype=dtype,
                            cpad=cpad, fork=fork)
    if fork is not None:
        return (out[0], N, T, Ho, Wo), out[1]
    return (out, N, T, Ho, Wo)


def _temporal(fm, conv, bn, relu, dtype, residual=None, in_affine=None):
    """(3,1,1) conv + BN(+res)(+ReLU): a (kt,1) conv over the [T, H*W] view of each clip.  in_affine: fm holds the spatial
    half's convolution output and this is the BatchNorm (+ ReLU) between the halves (see _spatial(defer=True))."""
    y, N, T, H, W = fm
    kt, st, pt = conv.kernel_size[0], conv.stride[0], conv.padding[0]
    out = F.conv_bn_act_raw(y, conv.weight, bn, (N, y.shape[1], T, H * W, False), (kt, 1), (st, 1), (pt, 0),
                            relu=relu, residual=residual, dtype=dtype, cpad=CPAD, in_affine=in_affine)
    To = (T + 2 * pt - kt) // st + 1
    return (out, N, To, H, W)


def _virtual_bn_pair(pair, N, T, H, W, dtype) -> bool:
    """Can the BatchNorm + ReLU between the two halves of this Conv2Plus1D stay virtual?  Needs the window kernels of the
    temporal half (144 mid planes -> 64, (3, 1, 1) / 1 / pad 1, a segment length that fits) and un-padded mid planes."""
    sp, tm = pair[0], pair[3]
    return bool(F.HALO_CONV and sp.out_channels == 144 and tm.in_channels == 144 and tm.out_channels == 64
                and tuple(sp.stride) == (1, 1, 1) and F.is_3x1_temporal((tm.kernel_size[0], 1), (tm.stride[0], 1), (tm.padding[0], 0))
                and _mid_cpad(sp, N * T, H, W, dtype) == 16            # (144 stays 144 only on the streamed-weight path)
                and ops.conv3x1_window_geometry(N, T, H * W, 144, 64, dtype))


class Conv3DSimple(nn.Conv3d):
    """Full 3x3x3 convolution (torchvision.models.video.resnet.Conv3DSimple)."""

    def __init__(self, in_planes, out_planes, midplanes=None, stride=1, padding=1):
        super().__init__(in_planes, out_planes, kernel_size=(3, 3, 3), stride=stride, padding=padding, bias=False)

    @staticmethod
    def get_downsample_stride(stride):
        return stride, stride, stride


# Kernel of each layer-1 half on the folded route where both dvt_conv2p1d_l1 and dvt_conv3d_implicit take it (16-bit), the
# faster one as measured on the MI355X at the reference test step: "spatial" = 64 -> 144 (1,3,3),
# "temporal" = 144 -> 64 (3,1,1).
L1_ROUTES = {"spatial": "l1", "temporal": "l1"}


def _route(fm, conv, dtype):
    """One of F.CONV3D_ROUTES for this convolution of the folded route."""
    if dtype not in (torch.bfloat16, torch.float16) or conv.in_channels not in (64, 144):
        return "implicit"
    y, N, T, H, W = fm
    k, s, p = tuple(conv.kernel_size), tuple(conv.stride), tuple(conv.padding)
    if y.shape[1] != conv.in_channels or not ops.conv2p1d_l1_supported(y, (N, T, H, W), conv.out_channels, k, s, p):
        return "implicit"
    return L1_ROUTES["spatial" if k[0] == 1 else "temporal"]


def _conv3d(fm, conv, bn, relu, dtype, residual=None, cout_multiple=1, route="implicit"):
    """conv3d -> eval BN (-> + residual) (-> ReLU) on an NDHWC matrix, one launch (F.conv3d_bn_act)."""
    y, N, T, H, W = fm
    out, To, Ho, Wo = F.conv3d_bn_act(y, conv, bn, (N, T, H, W), relu=relu, residual=residual, dtype=dtype,
                                      cout_multiple=cout_multiple, route=route)
    return (out, N, To, Ho, Wo)


def _folded_pair(fm, pair, bn, relu, dtype, residual=None):
    """Conv2Plus1D -> BN (-> + residual) (-> ReLU) of the inference route: the spatial half with the mid BatchNorm + ReLU
    folded (mid planes 45 / 230 / 460 / 921 carried as 48 / 232 / 464 / 928, the extra planes zero), then the temporal half
    with the block's BatchNorm, shortcut and ReLU folded -- two launches."""
    mid = _conv3d(fm, pair[0], pair[1], True, dtype, cout_multiple=8, route=_route(fm, pair[0], dtype))
    return _conv3d(mid, pair[3], bn, relu, dtype, residual=residual, route=_route(mid, pair[3], dtype))


# Compute dtypes in which eval() under torch.inference_mode() takes the folded route.  Measured on the MI355X at the reference
# test step (28 clips of 12 x 112^2), encoder alone: fp32 24.5 ms folded vs 78.4 ms on the eval() + no_grad
# route; bf16 5.26 ms folded (layer 1 on dvt_conv2p1d_l1) vs 3.69 ms -- in 16 bits the training route's layer-specialised
# halo / window / streamed-weight kernels still win layer 1 and the stem, so 16-bit inference keeps that route
# (VideoResNet.features_folded runs the folded one in any dtype).
FOLDED_ROUTE_DTYPES = (torch.float32,)


def inference_route(module: nn.Module) -> bool:
    """The folded inference route of an R(2+1)D VideoResNet runs in eval() under torch.inference_mode() (Lightning's
    test / predict) where it is the faster one (FOLDED_ROUTE_DTYPES); eval() under torch.no_grad() and training keep the
    training kernels' route."""
    return (not module.training and torch.is_inference_mode_enabled()
            and getattr(module, "compute_dtype", None) in FOLDED_ROUTE_DTYPES)


class BasicBlock(nn.Module):
    expansion = 1

    def __init__(self, inplanes, planes, conv_builder, stride=1, downsample=None):
        midplanes = (inplanes * planes * 3 * 3 * 3) // (inplanes * 3 * 3 + 3 * planes)
        super().__init__()
        self.conv1 = nn.Sequential(conv_builder(inplanes, planes, midplanes, stride), nn.BatchNorm3d(planes),
                                   nn.ReLU(inplace=True))
        self.conv2 = nn.Sequential(conv_builder(planes, planes, midplanes), nn.BatchNorm3d(planes))
        self.relu = nn.ReLU(inplace=True)
        self.downsample = downsample
        self.stride = stride

    def forward_ndhwc(self, fm, dtype):
        if isinstance(self.conv1[0], nn.Conv3d):                   # Conv3DSimple (r3d_18): inference path
            return self._forward_3d(fm, dtype)
        y, N, T, H, W = fm
        c1, c2 = self.conv1[0], self.conv2[0]
        if _virtual_bn_pair(c1, N, T, H, W, dtype):
            # the spatial half leaves its output z; the BatchNorm + ReLU between the halves runs inside the temporal half's kernels
            out, y, aff = _spatial(fm, c1[0], c1[1], True, dtype, fork="alias", defer=True)
            out = _temporal(out, c1[3], self.conv1[1], True, dtype, in_affine=aff)
        else:
            out, y = _spatial(fm, c1[0], c1[1], True, dtype, fork="alias")      # y: the block input again, for the shortcut
            out = _temporal(out, c1[3], self.conv1[1], True, dtype)
        residual = y
        if self.downsample is not None:
            ds, dbn = self.downsample[0], self.downsample[1]
            st = ds.stride
            C = ds.in_channels
            r = F.subsample_nhwc(y, N * T, C, H, W, (st[1], st[2]))                       # spatial stride
            Hs, Ws = (H - 1) // st[1] + 1, (W - 1) // st[2] + 1
            r = F.subsample_nhwc(r, N, C, T, Hs * Ws, (st[0], 1))                        # temporal stride
            Ts = (T - 1) // st[0] + 1
            residual = F.conv_bn_act_raw(r, ds.weight, dbn, (N * Ts, C, Hs, Ws, False), 1, 1, 0, relu=False, dtype=dtype)
        _, N2, T2, H2, W2 = out
        if _virtual_bn_pair(c2, N2, T2, H2, W2, dtype):
            out, _, aff = _spatial(out, c2[0], c2[1], True, dtype, defer=True)
            return _temporal(out, c2[3], self.conv2[1], True, dtype, residual=residual, in_affine=aff)
        out = _spatial(out, c2[0], c2[1], True, dtype)
        return _temporal(out, c2[3], self.conv2[1], True, dtype, residual=residual)     # out += residual; relu

    def forward_folded(self, fm, dtype):
        """Inference route of an R(2+1)D block: every convolution one dvt_conv3d_implicit launch with its BatchNorm (and
        the shortcut add and ReLU of the block's end) in the epilogue."""
        out = _folded_pair(fm, self.conv1[0], self.conv1[1], True, dtype)
        residual = fm[0]
        if self.downsample is not None:
            residual = _conv3d(fm, self.downsample[0], self.downsample[1], False, dtype)[0]
        return _folded_pair(out, self.conv2[0], self.conv2[1], True, dtype, residual=residual)     # out += residual; relu

    def _forward_3d(self, fm, dtype):
        out = _conv3d(fm, self.conv1[0], self.conv1[1], True, dtype)
        residual = fm[0]
        if self.downsample is not None:
            residual = _conv3d(fm, self.downsample[0], self.downsample[1], False, dtype)[0]
        return _conv3d(out, self.conv2[0], self.conv2[1], True, dtype, residual=residual)     # out += residual; relu


class BasicStem(nn.Sequential):
    """Conv3d(3, 64, (3, 7, 7), (1, 2, 2), (1, 3, 3)) -> BN -> ReLU (torchvision.models.video.resnet.BasicStem)."""

    def __init__(self):
        super().__init__(
            nn.Conv3d(3, 64, kernel_size=(3, 7, 7), stride=(1, 2, 2), padding=(1, 3, 3), bias=False),
            nn.BatchNorm3d(64), nn.ReLU(inplace=True))


class R2Plus1dStem(nn.Sequential):
    def __init__(self):
        super().__init__(
            nn.Conv3d(3, 45, kernel_size=(1, 7, 7), stride=(1, 2, 2), padding=(0, 3, 3), bias=False),
            nn.BatchNorm3d(45), nn.ReLU(inplace=True),
            nn.Conv3d(45, 64, kernel_size=(3, 1, 1), stride=(1, 1, 1), padding=(1, 0, 0), bias=False),
            nn.BatchNorm3d(64), nn.ReLU(inplace=True))


def _clip_ndhwc8(x, dt):
    """[N, 3, T, H, W] -> NDHWC [N*T*H*W, 8] in the compute dtype, planes 3..7 zero (the kernel's 16-byte channel chunks).
    x may also be the [N, T, 3, H, W] clip stack permuted (FrameTransformer.vid_step): its per-frame planes are read as
    they lie."""
    N, _, T, H, W = x.shape
    frames = x.permute(0, 2, 1, 3, 4)
    src = frames.reshape(N * T, 3, H, W) if frames.is_contiguous() and not x.is_contiguous() else x.reshape(N, 3, T * H, W)
    if dt in (torch.bfloat16, torch.float16):
        return ops.nchw_to_nhwc_pad(src, dt, 8)
    src = src.reshape(src.shape[0], 3, -1)                       # (the one-pass form writes 16-bit maps only)
    xt = ops.transpose_last2(src if src.dtype == dt else ops.cast(src, dt))
    y = ops.zeros((N * T * H * W, 8), dt, x.device)
    ops.copy2d(xt, y, N * T * H * W, 3, 3, 8)
    return y


class VideoResNet(nn.Module):
    """block / conv_makers / stem: torchvision's VideoResNet arguments (defaults: R(2+1)D-18)."""

    # class-activation tap (dvt_amd/cam.py): the name of one block ("layer4.1") whose output ``features`` makes a leaf of the
    # autograd graph and leaves in ``cam_tapped``; None (always, outside a CAM call): ``features`` runs as it does without one
    cam_tap = None
    cam_tapped = None

    def __init__(self, layers=(2, 2, 2, 2), num_classes=400, *, compute_dtype=torch.bfloat16, block=None, conv_makers=None,
                 stem=None):
        super().__init__()
        block = BasicBlock if block is None else block
        conv_makers = [Conv2Plus1D] * 4 if conv_makers is None else list(conv_makers)
        self.inplanes = 64
        self.stem = R2Plus1dStem() if stem is None else stem()
        self.layer1 = self._make_layer(64, layers[0], 1, block, conv_makers[0])
        self.layer2 = self._make_layer(128, layers[1], 2, block, conv_makers[1])
        self.layer3 = self._make_layer(256, layers[2], 2, block, conv_makers[2])
        self.layer4 = self._make_layer(512, layers[3], 2, block, conv_makers[3])
        self.avgpool = nn.AdaptiveAvgPool3d((1, 1, 1))
        self.fc = nn.Linear(512, num_classes)
        self.compute_dtype = compute_dtype
        for m in self.modules():
            if isinstance(m, nn.Conv3d):
                nn.init.kaiming_normal_(m.weight, mode="fan_out", nonlinearity="relu")
            elif isinstance(m, nn.BatchNorm3d):
                nn.init.constant_(m.weight, 1)
                nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.Linear):
                nn.init.normal_(m.weight, 0, 0.01)
                nn.init.constant_(m.bias, 0)

    def _make_layer(self, planes, blocks, stride, block=BasicBlock, conv_builder=Conv2Plus1D):
        downsample = None
        if stride != 1 or self.inplanes != planes * block.expansion:
            ds = conv_builder.get_downsample_stride(stride)
            downsample = nn.Sequential(nn.Conv3d(self.inplanes, planes * block.expansion, kernel_size=1, stride=ds, bias=False),
                                       nn.BatchNorm3d(planes * block.expansion))
        layers = [block(self.inplanes, planes, conv_builder, stride, downsample)]
        self.inplanes = planes * block.expansion
        for _ in range(1, blocks):
            layers.append(block(self.inplanes, planes, conv_builder))
        return nn.Sequential(*layers)

    def features(self, x):
        """x [N, 3, T, H, W] -> pooled [N, 512]."""
        if x.dim() != 5 or x.shape[1] != 3:
            raise ValueError("VideoResNet expects clips [N, 3, T, H, W]")
        if self.cam_tap is not None:
            return self._features_tapped(x)
        if isinstance(self.stem, BasicStem):
            return self._features_3d(x)
        if inference_route(self):
            return self.features_folded(x)
        fm = self._stem_ndhwc(x)
        dt = self.compute_dtype
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                fm = blk.forward_ndhwc(fm, dt)
        y, N, T, H, W = fm
        return F.mean_rows(y.view(N, T * H * W, y.shape[1]))          # AdaptiveAvgPool3d(1)

    def _stem_ndhwc(self, x):
        """R2Plus1dStem on the training kernels' route: clips [N, 3, T, H, W] -> the NDHWC map (y, N, T, H1, W1)."""
        dt = self.compute_dtype
        N, _, T, H, W = x.shape
        frames = x.permute(0, 2, 1, 3, 4)                  # [N, T, 3, H, W]: per-frame NCHW
        if not frames.is_contiguous():
            frames = frames.contiguous()
        s0, b0, s3, b3 = self.stem[0], self.stem[1], self.stem[3], self.stem[4]
        k, s, p = s0.kernel_size[1:], s0.stride[1:], s0.padding[1:]
        # input_grad_clips: indices of the clips whose pixel gradient is consumed (None = all): the caller's hint that
        # only the learnable CLS clip of each sample needs d(loss)/d(pixels)
        hint = getattr(self, "input_grad_clips", None)
        dx_frames = None if hint is None else [(int(c) * T, T) for c in hint]
        y = F.conv_bn_act_raw(frames.view(N * T, 3, H, W), s0.weight, b0, (N * T, 3, H, W, True), k, s, p, relu=True, dtype=dt,
                              cpad=CPAD, dx_frames=dx_frames)
        H1, W1 = (H + 2 * p[0] - k[0]) // s[0] + 1, (W + 2 * p[1] - k[1]) // s[1] + 1
        return _temporal((y, N, T, H1, W1), s3, b3, True, dt)

    def _features_tapped(self, x):
        """``features`` with a class-activation tap (dvt_amd/cam.py): ``cam_tap`` names a block ("layer4.1").  Everything up to
        and including that block runs without autograd; the block's output becomes a leaf and is left, with its geometry, in
        ``cam_tapped`` = (y [N*T*H*W, C], N, T, H, W); the rest runs with autograd.  A backward from the result therefore stops
        at the tap: nothing upstream is saved and no weight gradient is formed upstream."""
        if isinstance(self.stem, BasicStem):
            raise NotImplementedError("cam_tap: only the R(2+1)D tree carries a class-activation tap (r3d_18 does not)")
        if self.training:
            raise RuntimeError("cam_tap: class-activation maps are taken on running statistics: put the module in eval()")
        blocks = [(f"layer{i + 1}.{j}", blk) for i, layer in enumerate((self.layer1, self.layer2, self.layer3, self.layer4))
                  for j, blk in enumerate(layer)]
        names = [n for n, _ in blocks]
        if self.cam_tap not in names:
            raise ValueError(f"cam_tap {self.cam_tap!r} names no block of this network (one of {names})")
        cut = names.index(self.cam_tap) + 1
        dt = self.compute_dtype
        with torch.no_grad():
            fm = self._stem_ndhwc(x)
            for _, blk in blocks[:cut]:
                fm = blk.forward_ndhwc(fm, dt)
        y, N, T, H, W = fm
        y = y.detach().requires_grad_()
        self.cam_tapped = fm = (y, N, T, H, W)
        with torch.enable_grad():
            for _, blk in blocks[cut:]:
                fm = blk.forward_ndhwc(fm, dt)
            out, N, T, H, W = fm
            return F.mean_rows(out.view(N, T * H * W, out.shape[1]))          # AdaptiveAvgPool3d(1)

    def _features_3d(self, x):
        """Full-3-D tree (r3d_18): every convolution one dvt_conv3d_implicit launch; eval mode, no autograd."""
        if self.training:
            raise NotImplementedError("r3d_18 is an inference-only feature extractor here (no training / backward path): "
                                      "call .eval() and run it under torch.no_grad()")
        dt = self.compute_dtype
        N, _, T, H, W = x.shape
        y = _clip_ndhwc8(x, dt)
        fm = _conv3d((y, N, T, H, W), self.stem[0], self.stem[1], True, dt)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                fm = blk.forward_ndhwc(fm, dt)
        y, N, T, H, W = fm
        return F.mean_rows(y.view(N, T * H * W, y.shape[1]))          # AdaptiveAvgPool3d(1)

    def features_folded(self, x):
        """R(2+1)D folded inference route (what ``features`` runs in eval() under torch.inference_mode(), see
        inference_route; callable directly in any compute dtype, eval mode, no autograd): every Conv3d -> BatchNorm3d
        (-> + shortcut) (-> ReLU) of the stem, the four layers and the downsamples is one dvt_conv3d_implicit launch with
        the running statistics folded into its epilogue; weights are packed and BatchNorm folded once per module
        (F._conv3d_pack)."""
        if self.training:
            raise RuntimeError("features_folded folds the running statistics: put the module in eval()")
        dt = self.compute_dtype
        N, _, T, H, W = x.shape
        fm = (_clip_ndhwc8(x, dt), N, T, H, W)
        fm = _folded_pair(fm, self.stem, self.stem[4], True, dt)
        for layer in (self.layer1, self.layer2, self.layer3, self.layer4):
            for blk in layer:
                fm = blk.forward_folded(fm, dt)
        y, N, T, H, W = fm
        return F.mean_rows(y.view(N, T * H * W, y.shape[1]))          # AdaptiveAvgPool3d(1)

    def forward(self, x):
        feats = self.features(x)
        fc = self.fc[0] if isinstance(self.fc, nn.Sequential) else self.fc
        if not hasattr(fc, "weight"):                                # fc = Identity(): the pooled features (the expert)
            return feats
        return F.linear(feats, fc.weight, fc.bias)


def r2plus1d_18(pretrained=False, **kwargs):
    if pretrained:
        raise RuntimeError("pretrained=True downloads Kinetics weights (torchvision); there is no network here -- "
                           "load a state_dict explicitly")
    return VideoResNet((2, 2, 2, 2), **kwargs)


def r3d_18(pretrained=False, **kwargs):
    """torchvision.models.video.r3d_18: 3x3x3 convolutions throughout, inference only."""
    if pretrained:
        raise RuntimeError("pretrained=True downloads Kinetics weights (torchvision); there is no network here -- "
                           "load a state_dict explicitly")
    return VideoResNet((2, 2, 2, 2), block=BasicBlock, conv_makers=[Conv3DSimple] * 4, stem=BasicStem, **kwargs)
