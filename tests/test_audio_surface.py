"""CPU-side checks of the VGGish audio expert: the float64 restatement of the log-mel front end (tests/audio_ref.py) against
its fixture and against properties that follow from the definition, the frame and example counts (restatement and library),
the module's state-dict keys, seeded init and refusals, the extractor's opt-in, and the exported entry points."""
import math

import numpy as np
import pytest
import torch

from tests import audio_ref as A
from tests.util import golden


def test_restatement_reproduces_the_fixture():
    g = golden("audio_logmel.npz")
    wave = A.seeded_waveform(int(g["seed"]))
    assert np.array_equal(wave[:8], g["wave_head"])              # the generator still yields the stored waveform
    got = A.logmel_examples(wave)
    assert got.shape == g["logmel"].shape == (1, 96, 64) and got.dtype == np.float64
    assert np.abs(got - g["logmel"]).max() <= 1e-12


def test_mel_matrix_shape_of_the_definition():
    M = A.mel_matrix()
    assert M.shape == (257, 64) and M.min() >= 0.0 and M.max() <= 1.0
    assert np.all(M[0] == 0.0)                                    # the DC row
    for b in range(64):                                           # one triangle per band: its nonzero bins are contiguous
        nz = np.nonzero(M[:, b])[0]
        assert nz.size > 0 and np.array_equal(nz, np.arange(nz[0], nz[-1] + 1)), b
    edges = A.mel_edges()
    assert edges.shape == (66,) and np.allclose(np.diff(edges), np.diff(edges)[0], rtol=1e-12)
    assert math.isclose(edges[0], 1127.0 * math.log(1 + 125 / 700)) and math.isclose(edges[-1], 1127.0 * math.log(1 + 7500 / 700))
    # nothing at or above 7500 Hz (bin 240) or at or below 125 Hz (bin 4) carries weight
    assert np.all(M[240:] == 0.0) and np.all(M[:5] == 0.0) and M[5].sum() > 0 and M[239].sum() > 0


def test_a_1khz_tone_peaks_in_the_band_centred_nearest_1khz():
    t = np.arange(16000) / 16000.0
    lm = A.logmel_examples(0.5 * np.sin(2 * np.pi * 1000.0 * t))[0]
    centres = A.mel_edges()[1:-1]
    want = int(np.argmin(np.abs(centres - A.hz_to_mel(1000.0))))
    assert np.all(np.argmax(lm, axis=1) == want)


def test_a_silent_clip_is_log_of_the_offset_everywhere():
    lm = A.logmel_examples(np.zeros(16000))
    assert lm.shape == (1, 96, 64) and np.all(lm == math.log(0.01))


@pytest.mark.parametrize("L,F,E", [(399, 0, 0), (400, 1, 0), (15599, 95, 0), (15600, 96, 1), (16000, 98, 1), (31000, 192, 2)])
def test_frame_and_example_counts(L, F, E):
    from dvt_amd import ops
    assert A.num_frames(L) == F and A.num_examples(L) == E
    assert ops.logmel_num_examples(L) == E                        # the library's own count (host only)
    out = A.logmel_examples(np.zeros((2, L)))
    assert out.shape == (2 * E, 96, 64)                           # empty with the right trailing dims, not an error


def test_library_tables_are_the_restatements_rounded_once():
    """dvt_logmel_tables (float64 on the host, one rounding): the window and the mel matrix against tests/audio_ref.py."""
    from dvt_amd import ops
    tab = ops.logmel_tables_host().numpy()
    assert np.array_equal(tab[:400], A.hann().astype(np.float32))
    mel = tab[-15 * 4 * 256:].reshape(15, 4, 4, 16, 4)            # [16-bin block][16-band tile][g][band][j]: bin 16 kb + 4 g + j
    M = mel.transpose(0, 2, 4, 1, 3).reshape(240, 64)
    want = A.mel_matrix()[:240]
    assert np.abs(M - want).max() <= 2.0 ** -24 and np.array_equal(M == 0, want == 0)


def test_state_dict_keys_and_pproc_keys_ignored(capsys):
    from dvt_amd.models.pretrained import VGGish, vggish
    net = vggish()
    assert "seeded random init" in capsys.readouterr().err
    keys = [f"features.{i}.{p}" for i in (0, 3, 6, 8, 11, 13) for p in ("weight", "bias")]
    keys += [f"embeddings.{i}.{p}" for i in (0, 2, 4) for p in ("weight", "bias")]
    sd = net.state_dict()
    assert list(sd) == keys
    assert sd["features.0.weight"].shape == (64, 1, 3, 3) and sd["embeddings.0.weight"].shape == (4096, 12288)
    assert sd["embeddings.4.weight"].shape == (128, 4096)
    assert net.compute_dtype == torch.bfloat16 and not net.training
    assert all(float(sd[k].min()) > 0 and float(sd[k].max()) < 0.11 for k in keys if k.endswith("bias"))
    other = VGGish(compute_dtype=torch.float16)
    sd2 = dict(sd)
    sd2["features.3.bias"] = sd["features.3.bias"] + 1
    sd2["pproc._pca_matrix"], sd2["pproc._pca_means"] = torch.zeros(128, 128), torch.zeros(128, 1)
    other.load_state_dict(sd2)
    assert torch.equal(other.features[3].bias, sd2["features.3.bias"]) and list(other.state_dict()) == keys
    with pytest.raises(RuntimeError):
        other.load_state_dict({k: v for k, v in sd.items() if k != "embeddings.2.bias"})


def test_seeded_init_is_reproducible():
    from dvt_amd.models.pretrained import vggish
    a, b, c = vggish(), vggish(), vggish(seed=5)
    for (k, p), q in zip(a.state_dict().items(), b.state_dict().values()):
        assert torch.equal(p, q), k
    assert not torch.equal(a.features[0].weight, c.features[0].weight)


def test_refusals():
    from dvt_amd.models.pretrained import VGGish, vggish
    with pytest.raises(NotImplementedError, match="post-processor"):
        VGGish(postprocess=True)
    with pytest.raises(NotImplementedError, match="post-processor"):
        vggish(postprocess=True)
    with pytest.raises(ValueError):
        VGGish(compute_dtype=torch.float64)
    net = vggish()
    net.train()
    for call in (net, net.embed):
        with pytest.raises(NotImplementedError, match="inference-only"):
            call(torch.zeros(1, 96, 64))
    with pytest.raises(RuntimeError, match="no CPU path|need tensors on the GPU"):
        net.eval()(torch.zeros(1, 16000))                         # no CPU fall-back


def test_extractor_builds_the_audio_net_only_when_asked(tmp_path, capsys, monkeypatch):
    from dvt_amd.models.pretrained import VGGish, vggish
    from dvt_amd.models.pretrained.models import EmbeddingExtractor
    monkeypatch.setattr(EmbeddingExtractor, "_build", lambda self, name, factory, path: None)   # (the three other experts: not built here)
    ex = EmbeddingExtractor({"gpu": 0})
    assert ex.audio_net is None and "VGGish" not in capsys.readouterr().err
    with pytest.raises(NotImplementedError):
        ex.forward_audio(torch.zeros(1, 16000))
    with pytest.raises(NotImplementedError):
        ex.extract_audio(torch.zeros(1, 16000))
    assert ex.return_expert_for_key("audio", torch.zeros(1, 16000)) == []
    assert EmbeddingExtractor({"gpu": 0, "audio_net": False}).audio_net is None
    capsys.readouterr()

    ex = EmbeddingExtractor({"gpu": 0, "audio_net": True, "compute_dtype": "fp16"})
    assert "VGGish" in capsys.readouterr().err
    assert isinstance(ex.audio_net, VGGish) and ex.audio_net.compute_dtype == torch.float16 and not ex.audio_net.training
    src = vggish(seed=9)
    assert not torch.equal(ex.audio_net.features[0].weight, src.features[0].weight)
    path = tmp_path / "vggish.pth"
    torch.save(dict(src.state_dict(), **{"pproc._pca_means": torch.zeros(128, 1)}), path)
    capsys.readouterr()
    ex = EmbeddingExtractor({"gpu": 0, "audio_net_weights": str(path)})
    assert "VGGish" not in capsys.readouterr().err                # a file: no warning
    assert torch.equal(ex.audio_net.embeddings[4].weight, src.embeddings[4].weight)


def test_header_exposes_the_entry_points():
    import ctypes as C
    import dvt_amd
    from dvt_amd import _lib, ops
    lib = dvt_amd._lib.load()
    names = ("dvt_logmel_num_examples", "dvt_logmel_examples_workspace_bytes", "dvt_logmel_tables", "dvt_logmel_examples",
             "dvt_vggish_conv1_pool")
    for name in names:
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert _lib.SIGNATURES["dvt_logmel_examples"][0] is C.c_int and len(_lib.SIGNATURES["dvt_logmel_examples"][1]) == 8
    assert len(_lib.SIGNATURES["dvt_vggish_conv1_pool"][1]) == 9
    assert _lib.ENUMS["dvt_logmel_variant"] == {"DVT_LOGMEL_DFT": 0, "DVT_LOGMEL_FFT": 1}
    assert ops.LOGMEL_VARIANT in ops.LOGMEL_VARIANTS
    assert lib.dvt_logmel_examples_workspace_bytes() == 4 * (400 + 512 + 25 * 30 * 256 + 15 * 4 * 256)
    assert _lib.ABI_VERSION == 5
    # argument checks come before any HIP call; an empty problem is a no-op whatever the pointers are
    p = 256
    assert lib.dvt_logmel_examples(None, 3, 15599, None, None, _lib.F32, 0, None) == 0
    assert lib.dvt_logmel_examples(None, 0, 16000, None, None, _lib.F32, 0, None) == 0
    assert lib.dvt_vggish_conv1_pool(None, None, None, None, 0, 96, 64, _lib.BF16, None) == 0
    checks = [
        ("dvt_logmel_examples", -1, lambda: lib.dvt_logmel_examples(None, 1, 16000, p, p, _lib.F32, 0, None)),
        ("dvt_logmel_examples", -1, lambda: lib.dvt_logmel_examples(p, 1, 16000, p + 4, p, _lib.F32, 0, None)),   # tables unaligned
        ("dvt_logmel_examples", -1, lambda: lib.dvt_logmel_examples(p, 1, 16000, p, p, _lib.F32, 2, None)),
        ("dvt_logmel_examples", -1, lambda: lib.dvt_logmel_examples(p, 1, 16000, p, p, 7, 0, None)),
        ("dvt_logmel_examples", -1, lambda: lib.dvt_logmel_examples(p, -1, 16000, p, p, _lib.F32, 0, None)),
        ("dvt_logmel_tables", -1, lambda: lib.dvt_logmel_tables(None, 1 << 20)),
        ("dvt_logmel_tables", -1, lambda: lib.dvt_logmel_tables(p, 16)),
        ("dvt_vggish_conv1_pool", -1, lambda: lib.dvt_vggish_conv1_pool(None, p, p, p, 1, 96, 64, _lib.F32, None)),
        ("dvt_vggish_conv1_pool", -1, lambda: lib.dvt_vggish_conv1_pool(p, p, p, p + 8, 1, 96, 64, _lib.F32, None)),
        ("dvt_vggish_conv1_pool", -2, lambda: lib.dvt_vggish_conv1_pool(p, p, p, p, 1, 96, 32, _lib.F32, None)),
        ("dvt_vggish_conv1_pool", -2, lambda: lib.dvt_vggish_conv1_pool(p, p, p, p, 1, 95, 64, _lib.F32, None)),
    ]
    for name, want, call in checks:
        assert call() == want and name.encode() in lib.dvt_last_error(), name
