"""The host side of the mel spectrogram without a GPU: the cached fp64 evaluations of the filterbank and of the DFT basis
(``hip_ops.mel_filterbank`` / ``mel_basis``) against a restatement written here and in tests/mel_cases.py, the two forms
of the restatement against each other, the fixture of tests/golden/make_mel_golden.py (the live reference's wiring), the
attributes of ``DeviceMelSpectrum`` and the limits.  Reads the fixture only."""
import math

import numpy as np
import pytest
import torch

import mel_cases as MC

CASES = MC.fixture_cases()
IDS = [c["name"] for c in CASES]


@pytest.mark.parametrize("n_fft,n_mels,sr", [(512, 120, 16000), (512, 40, 16000), (100, 8, 16000), (16, 3, 16000),
                                             (2048, 256, 44100)])
def test_filterbank_equals_the_restatement(n_fft, n_mels, sr):
    from brainmagick_amd import hip_ops as H
    fb, lo, hi = H.mel_filterbank(n_fft, n_mels, sr)
    want = MC.fbanks64(n_fft, n_mels, sr)
    assert fb.dtype == torch.float32 and tuple(fb.shape) == (n_fft // 2 + 1, n_mels)
    assert np.array_equal(fb.numpy(), want.astype(np.float32))              # equal after ONE rounding to fp32
    for m in range(n_mels):
        nz = np.flatnonzero(want[:, m].astype(np.float32))
        assert 0 <= lo[m] <= hi[m] <= n_fft // 2 + 1
        assert all(lo[m] <= b < hi[m] for b in nz), m                        # the range covers every non-zero weight
        assert (hi[m] - lo[m] == 0) == (len(nz) == 0)
    feeds = (fb.numpy() != 0).sum(1)
    assert feeds.max() <= 2                                                  # a bin feeds at most two rows
    assert H.mel_filterbank(n_fft, n_mels, sr)[0] is fb                      # cached


def test_the_empty_filter_of_120_mels():
    from brainmagick_amd import hip_ops as H
    _, lo, hi = H.mel_filterbank(512, 120, 16000)
    assert int((hi == lo).sum()) >= 1                # the case torchaudio warns about
    _, lo, hi = H.mel_filterbank(512, 40, 16000)
    assert int((hi == lo).sum()) == 0


@pytest.mark.parametrize("n_fft", [16, 100, 512])
@pytest.mark.parametrize("normalized", [True, False])
def test_basis_equals_the_restatement(n_fft, normalized):
    from brainmagick_amd import hip_ops as H
    basis = H.mel_basis(n_fft, normalized)
    nb = n_fft // 2 + 1
    assert basis.dtype == torch.float32 and tuple(basis.shape) == (n_fft, 2 * nb)
    w = [0.5 - 0.5 * math.cos(2 * math.pi * k / n_fft) for k in range(n_fft)]
    norm = math.sqrt(math.fsum(v * v for v in w)) if normalized else 1.0
    want = np.zeros((n_fft, 2 * nb))
    for k in range(n_fft):
        for b in range(nb):
            a = 2 * math.pi * ((k * b) % n_fft) / n_fft
            want[k, b], want[k, nb + b] = w[k] * math.cos(a) / norm, -w[k] * math.sin(a) / norm
    # one rounding to fp32 of values that agree to a few fp64 ulp (numpy's and libm's cos, sum against fsum): a value
    # that sits within 1e-15 of a rounding boundary may land on either side
    diff = np.abs(basis.numpy().astype(np.float64) - want.astype(np.float32).astype(np.float64))
    assert (diff <= np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)).all()
    assert (diff == 0).mean() > 0.999
    # ... and as a transform: a frame times the basis is the windowed DFT
    x = torch.randn(n_fft, generator=torch.Generator().manual_seed(n_fft), dtype=torch.float64)
    got = x @ basis.double()
    window = torch.hann_window(n_fft, periodic=True, dtype=torch.float64)
    ref = torch.fft.rfft(x * window) / (window.pow(2).sum().sqrt() if normalized else 1.0)
    assert torch.allclose(got[:nb], ref.real, rtol=0, atol=2e-6 * float(ref.abs().max()))
    assert torch.allclose(got[nb:], ref.imag, rtol=0, atol=2e-6 * float(ref.abs().max()))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_direct_dft_equals_torch_stft_in_fp64(case):
    mono = case["wave"].double().mean(0)
    a = MC.direct_mel(mono, case["n_fft"], case["n_mels"], case["in_sampling"], case["normalized"])
    b = MC.stft_mel(mono, case["n_fft"], case["n_mels"], case["in_sampling"], case["normalized"])
    assert a.shape == b.shape == case["out64"].shape
    assert float((a - b).abs().max()) <= 1e-12 * float(b.abs().max())


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture_is_the_wiring_around_the_restatement(case):
    """mean over channels -> normalisation -> transform -> log, recomputed here in both precisions with the same torch
    ops in the same order as the live reference's ``_compute`` recorded them: equal up to the order of the CPU's
    reductions (the fixture is made with one thread), far below any difference in the wiring."""
    for dtype, key in ((torch.float32, "out32"), (torch.float64, "out64")):
        wav = torch.mean(case["wave"].to(dtype), dim=0)
        if case["norm_audio"]:
            wav = (wav - wav.mean()) / (1e-8 + wav.std())
        mel = MC.stft_mel(wav, case["n_fft"], case["n_mels"], case["in_sampling"], case["normalized"])
        mel = MC.finish(mel, case["use_log_scale"], case["log_scale_eps"])
        assert torch.allclose(mel, case[key], rtol=1e-5 if dtype == torch.float32 else 1e-12, atol=1e-6)


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_fixture_fp32_is_within_the_tolerance_rule_of_its_fp64(case):
    """The reference side's own deviation is what the GPU tests scale their bound with: it must be a deviation of the
    size fp32 gives (not zero, not a wiring difference between the two records)."""
    dev = MC.deviation(case["out32"], case["out64"], case["use_log_scale"])
    assert 0 < dev < 1e-4, dev
    # the fp32 record against the fp64 one fed the fp32-normalised input: the reference-side deviation of the rule
    mono = torch.mean(case["wave"], dim=0)
    x = MC.normalise64(mono) if case["norm_audio"] else mono
    truth = MC.finish(MC.stft_mel(x.double(), case["n_fft"], case["n_mels"], case["in_sampling"], case["normalized"]),
                      case["use_log_scale"], case["log_scale_eps"])
    ref32 = MC.finish(MC.stft_mel(x, case["n_fft"], case["n_mels"], case["in_sampling"], case["normalized"]),
                      case["use_log_scale"], case["log_scale_eps"])
    ref_dev = MC.deviation(ref32, truth, case["use_log_scale"])
    assert MC.deviation(case["out32"], truth, case["use_log_scale"]) <= MC.TOL_FACTOR * ref_dev


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_device_mel_spectrum_attributes(case):
    from brainmagick_amd.audio import DeviceMelSpectrum
    kw = {k: case[k] for k in ("norm_audio", "use_log_scale", "normalized")}
    feature = DeviceMelSpectrum(120.0, n_mels=case["n_mels"], n_fft=case["n_fft"], in_sampling=case["in_sampling"], **kw)
    for name, want in case["attributes"].items():
        assert getattr(feature, name) == want, name
    ef = feature.feature()
    assert (ef.name, ef.rule, ef.event_kind, ef.dimension) == ("MelSpectrum", "resampled", "sound", case["n_mels"])
    assert ef.default_value == case["attributes"]["default_value"]


def test_defaults_are_the_reference_s():
    import inspect
    from brainmagick_amd.audio import DeviceMelSpectrum
    sig = inspect.signature(DeviceMelSpectrum)
    got = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert got == dict(n_mels=40, n_fft=512, in_sampling=16_000, normalized=True, use_log_scale=True, log_scale_eps=1e-5,
                       norm_audio=True)
    assert DeviceMelSpectrum(120.0).default_value == math.log10(1e-5) and DeviceMelSpectrum.event_kind == "sound"


def test_every_limit_raises_its_value_error():
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.audio import DeviceMelSpectrum
    wave = torch.zeros(4000)
    for kw, word in ((dict(n_fft=4), "n_fft"), (dict(n_fft=4096), "n_fft"), (dict(n_fft=510), "multiple of 4"),
                     (dict(n_mels=257), "n_mels"), (dict(n_mels=0), "n_mels")):
        with pytest.raises(ValueError, match=word):
            H.mel_spectrograms([wave], **kw)
        with pytest.raises(ValueError, match=word):
            DeviceMelSpectrum(120.0, **kw)
    with pytest.raises(ValueError, match="n_fft // 2"):
        H.mel_spectrograms([torch.zeros(256)], n_fft=512)                    # L > n_fft // 2, as torch's reflect pad
    with pytest.raises(ValueError, match=r"2\^31"):
        H.mel_spectrograms([torch.empty(2 ** 31, device="meta")])
    with pytest.raises(ValueError, match=r"2\^31"):
        H.wave_moments([torch.empty(2 ** 31, device="meta")])
    with pytest.raises(ValueError, match="limit is 65535"):
        H.mel_spectrograms([wave] * 65536)
    feature = DeviceMelSpectrum(120.0)
    with pytest.raises(ValueError, match="resampling"):
        feature.compute([wave], 44_100)
    with pytest.raises(ValueError, match="sample rates"):
        feature.compute([wave, wave], [16_000])
    with pytest.raises(RuntimeError):                                        # within the limits: no CPU fallback
        H.mel_spectrograms([wave])


def test_mel_kernels_use_no_scratch_and_no_atomics_in_the_spectrogram():
    """ISA audit on the cross-compiled unit: no kernel of mel.hip spills or has a private segment, the contraction is
    the exact-fp32 MFMA, and the spectrogram launch holds no atomic (the moments launch draws its ticket with one)."""
    import re
    import shutil
    import subprocess
    import tempfile
    from pathlib import Path
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = Path(__file__).resolve().parent.parent / "brainmagick_amd" / "csrc"
    with tempfile.TemporaryDirectory(prefix="bm_asm_") as tmp:
        out = Path(tmp) / "mel.s"
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{csrc}",
                        "-o", str(out), str(csrc / "mel.hip")], check=True, capture_output=True)
        text = out.read_text()
    bodies = dict(re.findall(r"^(_Z\d+\w*_kernel\w*):(.*?)^\.Lfunc_end", text, flags=re.M | re.S))
    assert len(bodies) == 3, sorted(bodies)                  # wave_moments, mel_spectrogram<1>, <2>
    for kname, body in bodies.items():
        assert "scratch_" not in body, kname
        if "mel_spectrogram" in kname:
            assert "v_mfma_f32_16x16x4_f32" in body and "atomic" not in body, kname
    spills = [int(l.split(":")[1]) for l in text.splitlines() if ".vgpr_spill_count" in l or ".sgpr_spill_count" in l]
    scratch = [int(l.split(":")[1]) for l in text.splitlines() if ".private_segment_fixed_size" in l]
    assert len(spills) == 6 and len(scratch) == 3
    assert all(s == 0 for s in spills) and all(s == 0 for s in scratch), (spills, scratch)


def test_library_declares_the_mel_entry_points():
    from brainmagick_amd import _lib
    L = _lib.lib()
    assert L.bm_version() >= 114
    assert {"bm_wave_moments", "bm_mel_spectrogram", "bm_wave_table_fill"} <= set(_lib.parse_header())
    from brainmagick_amd import hip_ops as H
    assert H.mel_frame_tile(512) == H.MEL_FRAME_TILE and H.mel_frame_tile(2048) == 16
    assert L.bm_wave_moments_splits(9) == 1 and L.bm_wave_moments_splits(70001) == 5
