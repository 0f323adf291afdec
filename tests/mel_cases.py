"""torchaudio's MelSpectrogram restated from its documentation (torchaudio itself is not part of this stack), and the
MelSpectrum wiring of bm/features/audio.py:61-76 around it, as the tests and tests/golden/make_mel_golden.py use them.

Two forms of the same transform:

- ``stft_mel``: ``torch.stft(x, n_fft, hop, win_length=n_fft, window=hann_window(n_fft, periodic=True), center=True,
  pad_mode="reflect", onesided=True)``, divided by ``sqrt(sum w^2)`` when ``normalized``, ``|.|^2``, times the
  filterbank -- in ``x``'s dtype.  In fp64 it is the truth of the GPU tests; in fp32 it is the "reference-side
  evaluation" whose own deviation from that truth scales their tolerance.
- ``direct_mel``: a windowed DFT as a matrix product over the reflect-padded signal, fp64 (what the kernel computes).
"""
import json
import math
from pathlib import Path

import numpy as np
import torch

GOLDEN = Path(__file__).resolve().parent / "golden" / "mel_spectrum.npz"
TOL_FACTOR = 4.0            # the project's margin for an fp32 result against the reference's own fp32 deviation


def hz_to_mel(f: float) -> float:
    return 2595.0 * math.log10(1.0 + f / 700.0)


def fbanks64(n_fft: int, n_mels: int, sr: int) -> np.ndarray:
    """``melscale_fbanks(n_fft // 2 + 1, 0, sr // 2, n_mels, sr, norm=None, mel_scale="htk")`` in fp64: [n_freqs, n_mels]."""
    n_freqs = n_fft // 2 + 1
    f_max = float(sr // 2)
    all_freqs = np.linspace(0.0, f_max, n_freqs)
    m_pts = np.linspace(hz_to_mel(0.0), hz_to_mel(f_max), n_mels + 2)
    f_pts = 700.0 * (10.0 ** (m_pts / 2595.0) - 1.0)
    fb = np.zeros((n_freqs, n_mels))
    for m in range(n_mels):
        down = (all_freqs - f_pts[m]) / (f_pts[m + 1] - f_pts[m])
        up = (f_pts[m + 2] - all_freqs) / (f_pts[m + 2] - f_pts[m + 1])
        fb[:, m] = np.maximum(0.0, np.minimum(down, up))
    return fb


def stft_power(x: torch.Tensor, n_fft: int, normalized: bool) -> torch.Tensor:
    """[n_freqs, frames] in ``x``'s dtype."""
    window = torch.hann_window(n_fft, periodic=True, dtype=x.dtype)
    spec = torch.stft(x, n_fft, hop_length=n_fft // 4, win_length=n_fft, window=window, center=True, pad_mode="reflect",
                      normalized=False, onesided=True, return_complex=True)
    if normalized:
        spec = spec / window.pow(2.).sum().sqrt()
    return spec.abs().pow(2.)


def stft_mel(x: torch.Tensor, n_fft: int, n_mels: int, sr: int, normalized: bool) -> torch.Tensor:
    """[n_mels, frames] in ``x``'s dtype (the filterbank is evaluated in fp64 and rounded once to it)."""
    fb = torch.from_numpy(fbanks64(n_fft, n_mels, sr)).to(x.dtype)
    return torch.matmul(stft_power(x, n_fft, normalized).transpose(-1, -2), fb).transpose(-1, -2)


def direct_power(x: torch.Tensor, n_fft: int, normalized: bool) -> torch.Tensor:
    """[n_freqs, frames] fp64: the DFT of every frame of the reflect-padded signal as one matrix product."""
    x = x.double()
    hop, half, L = n_fft // 4, n_fft // 2, x.numel()
    idx = torch.arange(-half, L + half)
    idx = torch.where(idx < 0, -idx, idx)
    idx = torch.where(idx >= L, 2 * (L - 1) - idx, idx)
    padded = x[idx]
    frames = padded.unfold(0, n_fft, hop)                                           # [frames, n_fft]
    k = torch.arange(n_fft, dtype=torch.int64)
    w = 0.5 - 0.5 * torch.cos(2.0 * math.pi * k.double() / n_fft)
    norm = float(torch.sqrt((w * w).sum())) if normalized else 1.0
    angle = 2.0 * math.pi * ((k[:, None] * torch.arange(n_fft // 2 + 1)[None, :]) % n_fft).double() / n_fft
    re = frames @ (w[:, None] * torch.cos(angle) / norm)
    im = frames @ (-w[:, None] * torch.sin(angle) / norm)
    return (re * re + im * im).t()


def direct_mel(x: torch.Tensor, n_fft: int, n_mels: int, sr: int, normalized: bool) -> torch.Tensor:
    return torch.from_numpy(fbanks64(n_fft, n_mels, sr)).t() @ direct_power(x, n_fft, normalized)


def normalise64(mono: torch.Tensor) -> torch.Tensor:
    """``(wav - wav.mean()) / (1e-8 + wav.std())`` from fp64 statistics, rounded once to fp32."""
    d = mono.double()
    return ((d - d.mean()) / (1e-8 + d.std())).float()


_fixture = None


def fixture_cases():
    """tests/golden/mel_spectrum.npz, read once: a list of ``{name, n_fft, n_mels, L, in_sampling, norm_audio,
    use_log_scale, normalized, log_scale_eps, attributes, wave [2, L] fp32, out32, out64}``."""
    global _fixture
    if _fixture is None:
        z = np.load(GOLDEN)
        cases = json.loads(str(z["meta"]))["cases"]
        for c in cases:
            wave = z[c["wave"]].copy()
            if c["silence"]:
                wave[:, c["silence"][0]:c["silence"][1]] = 0.0
            c["wave"] = torch.from_numpy(wave)
            c["out32"] = torch.from_numpy(z[f"{c['name']}/out32"])
            c["out64"] = torch.from_numpy(z[f"{c['name']}/out64"])
        _fixture = cases
    return _fixture


def finish(mel: torch.Tensor, use_log_scale: bool, eps: float) -> torch.Tensor:
    return torch.log10(mel + eps) if use_log_scale else mel


def deviation(got: torch.Tensor, truth: torch.Tensor, use_log_scale: bool) -> float:
    """The tolerance rule's measure: the largest absolute deviation of the log output; without the logarithm the largest
    per-frame deviation divided by that frame's total power (frames of no power must be exact)."""
    diff = (got.double() - truth.double()).abs()
    if use_log_scale:
        return float(diff.max())
    total = truth.double().sum(0)
    live = total > 0
    assert bool((diff[:, ~live] == 0).all())
    return float((diff[:, live].max(0).values / total[live]).max()) if bool(live.any()) else 0.0
