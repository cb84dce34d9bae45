"""The VGGish audio expert on the MI355X: the log-mel front end against the float64 restatement (tests/audio_ref.py), the
fused first layer exactly, the whole network against the CPU stack, and the EmbeddingExtractor's audio key.

Every test prints its figures before it asserts; DESIGN 4.16 records them."""
import functools
import math

import numpy as np
import pytest
import torch

from tests import audio_ref as A
from tests.util import rel_l2

pytestmark = pytest.mark.gpu

LENGTHS = (15600, 16000, 31000)
MODES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}


def _clips(L):
    """R = 3: noise plus tones, a silent clip, a clip with most amplitudes at +-1."""
    rng = np.random.default_rng(L)
    t = np.arange(L) / A.SAMPLE_RATE
    loud = np.clip(5.0 * np.sin(2 * np.pi * 220.0 * t) + 0.5 * rng.standard_normal(L), -1.0, 1.0).astype(np.float32)
    assert (np.abs(loud) == 1.0).mean() > 0.5
    return np.stack([A.seeded_waveform(L, L), np.zeros(L, dtype=np.float32), loud])


@functools.lru_cache(maxsize=None)
def _front_end_refs(L):
    """(waveforms, float64 restatement, max-abs deviation of the fp32 chain from it); computed once per length."""
    wave = _clips(L)
    r64 = A.logmel_examples(wave)
    r32 = A.logmel_examples(wave, np.float32)
    for a in (wave, r64):
        a.setflags(write=False)
    return wave, r64, float(np.abs(r32.astype(np.float64) - r64).max())


# ------------------------------------------------------------------ front end
@pytest.mark.parametrize("L", LENGTHS)
def test_front_end_fp32_within_four_times_the_fp32_chain(device, L):
    """Max-abs error over the log-mel values against the float64 restatement; the bound is four times the error of the same
    chain evaluated in fp32 on the CPU (the factor covers another, fixed summation order over the 400- and 257-term sums).
    Measured on the MI355X (kernel / the fp32 chain on that host / bound): L = 15600: 3.50e-6 / 4.11e-6 / 1.64e-5;
    L = 16000: 1.17e-5 / 1.05e-5 / 4.21e-5; L = 31000: 5.24e-6 / 3.82e-6 / 1.53e-5 (also in DESIGN 4.16)."""
    from dvt_amd import ops
    wave, r64, ref_err = _front_end_refs(L)
    got = ops.logmel_examples(torch.from_numpy(wave.copy()).to(device), torch.float32)
    assert got.shape == r64.shape == (3 * A.num_examples(L), 96, 64) and got.dtype == torch.float32
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - r64).max())
    print(f"logmel L={L}: kernel ({ops.LOGMEL_VARIANT}) max-abs error {err:.3e}, fp32 chain {ref_err:.3e}, bound {4 * ref_err:.3e}")
    assert ref_err > 0 and err <= 4 * ref_err
    assert r64.max() - r64.min() > 1e4 * ref_err                  # the values span far more than the tolerance


# The table DFT sums 400 products per bin strictly in order where the fp32 chain's FFT rounds log2(512) = 9 times per output:
# with independent roundings the error grows with the square root of the count, so its bound is the kept form's factor of four
# times sqrt(400 / 9).  A wrong table entry or k layout moves the values by their own size, orders of magnitude past it.
DFT_FACTOR = 4 * math.sqrt(400 / 9)


@pytest.mark.parametrize("L", LENGTHS)
def test_front_end_table_dft_form_within_its_stated_bound(device, L):
    """Measured on the MI355X: 9.01e-6, 1.09e-5, 8.36e-6 for the three lengths (bounds 1.10e-4, 2.80e-4, 1.02e-4)."""
    from dvt_amd import ops
    wave, r64, ref_err = _front_end_refs(L)
    got = ops.logmel_examples(torch.from_numpy(wave).to(device), torch.float32, "dft")
    err = float(np.abs(got.cpu().numpy().astype(np.float64) - r64).max())
    print(f"logmel L={L}: kernel (dft) max-abs error {err:.3e}, fp32 chain {ref_err:.3e}, bound {DFT_FACTOR * ref_err:.3e}")
    assert err <= DFT_FACTOR * ref_err


@pytest.mark.parametrize("variant", ["dft", "fft"])
@pytest.mark.parametrize("L", LENGTHS)
def test_front_end_silent_clip_and_repeatability(device, L, variant):
    from dvt_amd import ops
    wave, _, _ = _front_end_refs(L)
    x = torch.from_numpy(wave).to(device)
    got = ops.logmel_examples(x, torch.float32, variant)
    E = A.num_examples(L)
    # zeros stay zeros through the window, the spectrum and the mel product: log(0 + 0.01f), correctly rounded
    silent = np.float32(math.log(float(np.float32(0.01))))
    assert torch.equal(got[E:2 * E].cpu(), torch.full((E, 96, 64), float(silent)))
    again = ops.logmel_examples(x, torch.float32, variant)
    assert torch.equal(got.view(torch.int32), again.view(torch.int32))


@pytest.mark.parametrize("mode", ["bf16", "fp16"])
def test_front_end_16bit_output_is_the_fp32_output_rounded_to_nearest_even(device, mode):
    from dvt_amd import ops
    wave, _, _ = _front_end_refs(31000)
    x = torch.from_numpy(wave).to(device)
    f32 = ops.logmel_examples(x, torch.float32)
    low = ops.logmel_examples(x, MODES[mode])
    assert low.dtype == MODES[mode] and torch.equal(low.view(torch.int16), f32.to(MODES[mode]).view(torch.int16))


def test_front_end_shorter_than_one_example_is_empty(device):
    from dvt_amd import ops
    from dvt_amd.models.pretrained import vggish
    out = ops.logmel_examples(torch.zeros(3, 15599, device=device), torch.bfloat16)
    assert out.shape == (0, 96, 64) and out.dtype == torch.bfloat16
    net = vggish(compute_dtype=torch.float32).to(device)
    assert net(torch.zeros(2, 3, 15599, device=device)).shape == (2, 3, 0, 128)


# ------------------------------------------------------------------ conv1 + pool, exactly
@pytest.mark.parametrize("mode", ["fp32", "bf16"])
def test_conv1_pool_is_exact_on_integers(device, mode):
    """Integer inputs in [-4, 4], weights in [-2, 2], biases in [-3, 3]: every sum is exact in fp32 and bf16 (|z| <= 75), the
    ReLU clamps and the pool windows hold ties -- bitwise equal to torch on the CPU."""
    from dvt_amd import ops
    dtype = MODES[mode]
    g = torch.Generator().manual_seed(3)
    x = torch.randint(-4, 5, (2, 96, 64), generator=g).float()
    w = torch.randint(-2, 3, (64, 1, 3, 3), generator=g).float()
    b = torch.randint(-3, 4, (64,), generator=g).float()
    z = torch.nn.functional.conv2d(x[:, None].to(dtype), w.to(dtype), b.to(dtype), padding=1)
    assert torch.equal(z.float(), torch.nn.functional.conv2d(x[:, None].double(), w.double(), b.double(), padding=1).float())
    a = z.clamp_min(0)
    want = torch.nn.functional.max_pool2d(a, 2, 2)
    assert float((z < 0).float().mean()) > 0.2 and int((b < 0).sum()) > 0                      # the clamps matter
    win = a.float().unfold(2, 2, 2).unfold(3, 2, 2).reshape(2, 64, 48, 32, 4)
    assert int(((win == want.float()[..., None]).sum(-1) > 1).sum()) > 1000                    # ties inside the windows
    got = ops.vggish_conv1_pool(x.to(device=device, dtype=dtype), w.to(device), b.to(device))
    assert got.shape == (2 * 48 * 32, 64) and got.dtype == dtype
    assert torch.equal(got.cpu().float(), want.permute(0, 2, 3, 1).reshape(-1, 64).float())


# ------------------------------------------------------------------ the whole expert
@functools.lru_cache(maxsize=None)
def _expert_refs():
    """N = 3 examples (odd, below every tile size), the seeded init's state dict, and the CPU stack's outputs per mode."""
    from dvt_amd.models.pretrained import vggish
    ex = torch.from_numpy(np.concatenate([A.logmel_examples(A.seeded_waveform(s)) for s in (1, 2, 3)])).float()
    sd = {k: v.clone() for k, v in vggish(compute_dtype=torch.float32).state_dict().items()}
    refs = {m: A.stack_forward(sd, ex, dt).float() for m, dt in MODES.items()}
    return ex, sd, refs


@pytest.fixture(scope="module")
def expert(device):
    from dvt_amd.models.pretrained import vggish
    return vggish(compute_dtype=torch.float32).to(device)


@pytest.mark.parametrize("mode", list(MODES))
def test_whole_expert_against_the_cpu_stack(device, expert, mode):
    """fp32: rel-L2 <= 1e-3 against the CPU stack.  bf16 / fp16: within twice the CPU stack's own deviation, in that dtype,
    from its fp32 run on the same inputs.  Liveness: at least half of the 3 x 128 reference outputs are nonzero.
    Measured on the MI355X: fp32 1.24e-6; bf16 6.58e-3 (the CPU stack's own 6.30e-3); fp16 8.53e-4 (9.32e-4)."""
    ex, sd, refs = _expert_refs()
    ref = refs["fp32"]
    assert ref.shape == (3, 128) and float((ref != 0).float().mean()) >= 0.5
    expert.compute_dtype = MODES[mode]
    try:
        with torch.no_grad():
            got = expert.embed(ex.to(device))
    finally:
        expert.compute_dtype = torch.float32
    assert got.shape == (3, 128) and got.dtype == MODES[mode]
    err = rel_l2(got.float().cpu(), ref)
    if mode == "fp32":
        print(f"vggish fp32: rel L2 {err:.3e} (bar 1e-3)")
        assert err <= 1e-3
    else:
        cpu_dev = rel_l2(refs[mode], ref)
        print(f"vggish {mode}: rel L2 {err:.3e}, the CPU stack's own {cpu_dev:.3e} (bound {2 * cpu_dev:.3e})")
        assert cpu_dev > 0 and err <= 2 * cpu_dev


def test_checkpoint_round_trip_reproduces_the_embedding_bitwise(device, expert, tmp_path):
    from dvt_amd.models.pretrained import vggish
    ex, sd, _ = _expert_refs()
    x = ex.to(device)
    with torch.no_grad():
        want = expert.embed(x)
    path = tmp_path / "vggish.pth"
    torch.save(dict(sd, **{"pproc._pca_matrix": torch.zeros(128, 128)}), path)
    other = vggish(str(path), compute_dtype=torch.float32, seed=11).to(device)
    with torch.no_grad():
        got = other.embed(x)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ------------------------------------------------------------------ the extractor's audio key
@pytest.fixture(scope="module")
def extractor():
    from dvt_amd.models.pretrained.models import EmbeddingExtractor
    return EmbeddingExtractor({"gpu": 0, "audio_net": True, "compute_dtype": "fp32"})


def test_extractor_audio_key(device, extractor):
    wav = torch.from_numpy(A.seeded_waveform(5, 31000))
    out = extractor.return_expert_for_key("audio", wav)
    assert out.shape == (2, 128) and out.dtype == torch.float32 and not out.is_cuda
    assert torch.equal(out, extractor.forward_audio(wav))
    assert extractor.extract_audio(wav).is_cuda


def test_extractor_chunks_batch_independence_and_pyramid_interop(device, extractor):
    from dvt_amd.models.pyramid_vivit import PyramidViViT
    wav = torch.from_numpy(np.stack([A.seeded_waveform(s) for s in range(10, 18)])).view(2, 4, 16000)
    tokens = extractor.extract_audio(wav)
    assert tokens.shape == (2, 4, 128) and tokens.is_cuda
    alone = extractor.forward_audio(wav[1, 2])                                   # [16000] -> [1, 128]
    assert alone.shape == (1, 128)
    err = rel_l2(alone[0], tokens[1, 2].float().cpu())
    print(f"chunk alone vs in the batch: rel L2 {err:.3e}")
    assert err <= 1e-3
    net = PyramidViViT(64, 19, 2, dim=128, depth=1, heads=2, dim_head=64, audio_tokens=4, audio_dim=128,
                       compute_dtype=torch.bfloat16).to(device).eval()
    with torch.no_grad():
        logits = net(torch.randn(2, 2, 3, 64, 64, device=device), tokens)         # no reshape in between
    logits = logits[0] if isinstance(logits, (tuple, list)) else logits
    assert logits.shape == (2, 19) and bool(torch.isfinite(logits.float()).all())
