#!/usr/bin/env python3
"""Write tests/golden/audio_logmel.npz: the float64 log-mel example of one seeded one-second waveform (noise plus two tones),
as tests/audio_ref.py computes it.  Only the waveform's seed is stored; tests regenerate it with audio_ref.seeded_waveform.

    python tools/gen_golden_audio.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from tests import audio_ref  # noqa: E402

SEED = 20


def main():
    wave = audio_ref.seeded_waveform(SEED)
    logmel = audio_ref.logmel_examples(wave)
    assert logmel.shape == (1, 96, 64) and logmel.dtype == np.float64
    path = os.path.join(ROOT, "tests", "golden", "audio_logmel.npz")
    np.savez(path, seed=np.int64(SEED), logmel=logmel, wave_head=wave[:8])
    print(f"wrote {path}: {os.path.getsize(path)} bytes")


if __name__ == "__main__":
    main()
