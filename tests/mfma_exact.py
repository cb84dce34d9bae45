"""Operands on which a missing MFMA k-step cannot hide: for the exact tests of the kernels that mix 16x16x32 and 16x16x16
MFMAs on one accumulator (tests/test_gpu_mfma_exact.py) and the CPU proof that they are sensitive (tests/test_isa_hazards.py).

A k-step is one MFMA's slice of the reduction: a filter tap times a channel range.  The window forward (conv3x1_fwd.hip,
144 channels per tap) takes ranges of 32, 32, 32, 32 (16x16x32) and 16 (16x16x16) channels per tap; the streamed 3x3 kernel
(conv3x3_stream.hip, 48-channel chunks) takes 32 (16x16x32) and 16 (16x16x16) per chunk and tap.  The input has exactly one
1 per pixel and channel range (at a pixel-dependent channel), everything else 0; the weights are constant over a range, a
small positive integer per (output channel, tap, range).  Every k-step then adds its weight to every output whose tap reads
inside the map, all partial sums are integers far below 2^24, and the outputs are exact in bf16 (<= 256) and fp16.
"""
import torch

WINDOW_RANGES = [(0, 32), (32, 64), (64, 96), (96, 128), (128, 144)]


def stream_ranges(cin):
    return [r for c0 in range(0, cin, 48) for r in ((c0, c0 + 32), (c0 + 32, c0 + 48))]


def one_hot_input(npix, cin, ranges, seed=0):
    """[npix, cin] float64: per pixel one 1 inside every range, at a pixel-dependent channel"""
    g = torch.Generator().manual_seed(seed)
    x = torch.zeros(npix, cin, dtype=torch.float64)
    rows = torch.arange(npix)
    for lo, hi in ranges:
        x[rows, lo + torch.randint(0, hi - lo, (npix,), generator=g)] = 1.0
    return x


def window_weights(cout=64):
    """[cout, 144, 3, 1] float64: step (tap kt, range c) of output channel co weighs 1 + (5 kt + c + co) % 15 -- for every
    output channel the 15 k-steps weigh 1 .. 15, each a different amount (an interior output is 120)"""
    w = torch.zeros(cout, 144, 3, 1, dtype=torch.float64)
    for co in range(cout):
        for kt in range(3):
            for c, (lo, hi) in enumerate(WINDOW_RANGES):
                w[co, lo:hi, kt, 0] = 1 + (5 * kt + c + co) % 15
    return w


def stream_weights(cin, cout):
    """[cout, cin, 3, 3] float64: every k-step weighs 1, except that output channel co weighs step co % steps twice (an
    interior output is steps + 1 <= 109: 9 taps x 12 ranges at 288 channels)"""
    ranges = stream_ranges(cin)
    nsteps = 9 * len(ranges)
    w = torch.ones(cout, cin, 3, 3, dtype=torch.float64)
    for co in range(cout):
        s = co % nsteps
        tap, r = divmod(s, len(ranges))
        lo, hi = ranges[r]
        w[co, lo:hi, tap // 3, tap % 3] = 2
    return w


def kstep_partials(x, w, ranges, padding):
    """float64 restatement of the kernel's k-step split: one NCHW conv2d per (tap, channel range), the tap's filter element
    alone -> [(tap, range index, partial output)]; their sum is the whole convolution"""
    out = []
    kh, kw = w.shape[2], w.shape[3]
    for i in range(kh):
        for j in range(kw):
            for r, (lo, hi) in enumerate(ranges):
                wm = torch.zeros_like(w)
                wm[:, lo:hi, i, j] = w[:, lo:hi, i, j]
                out.append(((i, j), r, torch.nn.functional.conv2d(x, wm, None, 1, padding)))
    return out
