"""CPU restatement of the VGGish audio expert (the definition of the issue that added it is the contract; neither torchvggish
nor librosa is available to arbitrate): the log-mel front end in numpy -- float64 by default, with ``np.fft.rfft``, a
different algorithm from either of the kernel's -- and the VGG stack in ``torch.nn``."""
import numpy as np
import torch
import torch.nn as nn

SAMPLE_RATE = 16000
WIN, HOP, NFFT, BINS, MEL = 400, 160, 512, 257, 64
MEL_LO_HZ, MEL_HI_HZ = 125.0, 7500.0
LOG_OFFSET = 0.01
EX_FRAMES, EX_HOP = 96, 96


def num_frames(L):
    return 0 if L < WIN else 1 + (L - WIN) // HOP


def num_examples(L):
    F = num_frames(L)
    return 0 if F < EX_FRAMES else 1 + (F - EX_FRAMES) // EX_HOP


def hz_to_mel(f):
    return 1127.0 * np.log(1.0 + np.asarray(f, dtype=np.float64) / 700.0)


def mel_edges():
    """The 66 band edges, equally spaced in mel."""
    return np.linspace(hz_to_mel(MEL_LO_HZ), hz_to_mel(MEL_HI_HZ), MEL + 2)


def mel_matrix():
    """[257, 64] float64; the DC row is zero."""
    edges = mel_edges()
    m = hz_to_mel(np.arange(BINS) * (SAMPLE_RATE / 2.0) / (BINS - 1))[:, None]
    lo, ctr, hi = edges[None, :-2], edges[None, 1:-1], edges[None, 2:]
    w = np.maximum(0.0, np.minimum((m - lo) / (ctr - lo), (hi - m) / (hi - ctr)))
    w[0, :] = 0.0
    return w


def hann():
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(WIN) / WIN)


def logmel_frames(wave, dtype=np.float64):
    """wave [L] -> log-mel [F, 64], every step of the chain in ``dtype`` (float32: the fp32 chain whose distance from the
    float64 one sets the kernel's tolerance; its rfft is torch's single-precision one)."""
    wave = np.asarray(wave, dtype=dtype)
    F = num_frames(wave.shape[0])
    if F == 0:
        return np.zeros((0, MEL), dtype=dtype)
    idx = np.arange(F)[:, None] * HOP + np.arange(WIN)[None, :]
    frames = wave[idx] * hann().astype(dtype)
    padded = np.zeros((F, NFFT), dtype=dtype)
    padded[:, :WIN] = frames
    if dtype == np.float32:                                # (numpy's rfft computes in double whatever the input)
        spec = torch.fft.rfft(torch.from_numpy(padded), dim=1).numpy()
        assert spec.dtype == np.complex64
    else:
        spec = np.fft.rfft(padded, axis=1)
    mag = np.abs(spec).astype(dtype)
    mel = mag @ mel_matrix().astype(dtype)
    return np.log(mel + dtype(LOG_OFFSET)).astype(dtype)


def logmel_examples(wave, dtype=np.float64):
    """wave [R, L] (or [L]) -> [R * E, 96, 64]; leftover frames are dropped; E == 0 gives an empty array."""
    wave = np.atleast_2d(np.asarray(wave))
    E = num_examples(wave.shape[1])
    out = np.zeros((wave.shape[0] * E, EX_FRAMES, MEL), dtype=dtype)
    for r, row in enumerate(wave):
        lm = logmel_frames(row, dtype)
        for e in range(E):
            out[r * E + e] = lm[e * EX_HOP:e * EX_HOP + EX_FRAMES]
    return out


def seeded_waveform(seed, L=SAMPLE_RATE):
    """Noise plus two tones (440 Hz and 3 kHz), in [-1, 1]; float32, regenerated from its seed."""
    rng = np.random.default_rng(seed)
    t = np.arange(L) / SAMPLE_RATE
    x = 0.1 * rng.standard_normal(L) + 0.4 * np.sin(2 * np.pi * 440.0 * t) + 0.25 * np.sin(2 * np.pi * 3000.0 * t + 0.5)
    return np.clip(x, -1.0, 1.0).astype(np.float32)



# ---------------------------------------------------------------- the VGG stack
def make_stack():
    """(features, embeddings) of the public definition, in torch.nn, with the checkpoint's key names."""
    layers, cin = [], 1
    for v in (64, "M", 128, "M", 256, 256, "M", 512, 512, "M"):
        if v == "M":
            layers.append(nn.MaxPool2d(2, 2))
        else:
            layers += [nn.Conv2d(cin, v, 3, padding=1), nn.ReLU()]
            cin = v
    emb = nn.Sequential(nn.Linear(512 * 4 * 6, 4096), nn.ReLU(), nn.Linear(4096, 4096), nn.ReLU(), nn.Linear(4096, 128), nn.ReLU())
    return nn.Sequential(*layers), emb


def stack_forward(state_dict, examples, dtype=torch.float32):
    """examples [n, 96, 64] -> [n, 128] on the CPU: parameters and every activation in ``dtype``.  The public forward:
    features on [n, 1, 96, 64], NCHW -> NHWC, flatten, embeddings."""
    features, emb = make_stack()
    features.load_state_dict({k[len("features."):]: v for k, v in state_dict.items() if k.startswith("features.")})
    emb.load_state_dict({k[len("embeddings."):]: v for k, v in state_dict.items() if k.startswith("embeddings.")})
    features, emb = features.to(dtype).eval(), emb.to(dtype).eval()
    with torch.no_grad():
        y = features(examples.to(dtype)[:, None])
        y = y.permute(0, 2, 3, 1).reshape(y.shape[0], -1)
        return emb(y)
