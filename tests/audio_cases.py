"""julius' ``ResampleFrac`` and the YIN pitch of bm/lib/pitch_calc/yin.py restated, as the tests and
tests/golden/make_audio_rates_golden.py use them (julius and numba are not part of this stack).

- ``ResampleFrac``: julius' published definition in torch ops, in the dtype of the waveform it is handed (the taps are
  julius' own fp32 expressions, cast): the ``julius`` stub of the fixture maker, the fp64 truth and the fp32
  "reference-side evaluation" of the GPU tests.
- ``taps64``: the same table evaluated in fp64.
- ``yin_direct``: the pitches with the difference function as a direct fp64 sum (what the kernel computes; the
  reference forms it with an FFT), and the smallest margin of any comparison it took.
"""
import json
import math
from pathlib import Path

import numpy as np
import torch
from torch.nn import functional as F

GOLDEN = Path(__file__).resolve().parent / "golden" / "audio_rates.npz"


def reduced(old_sr: int, new_sr: int):
    g = math.gcd(int(old_sr), int(new_sr))
    return int(old_sr) // g, int(new_sr) // g


def taps_in(dtype, old_sr: int, new_sr: int, zeros: int = 24, rolloff: float = 0.945):
    """``(taps [new, 2 width + old], old, new, width)`` with every tensor expression in ``dtype``."""
    old, new = reduced(old_sr, new_sr)
    sr = min(old, new) * rolloff
    width = math.ceil(zeros * old / sr)
    idx = torch.arange(-width, width + old).to(dtype)
    rows = []
    for i in range(new):
        t = (-i / new + idx / old) * sr
        t.clamp_(-zeros, zeros)
        t *= math.pi
        window = torch.cos(t / zeros / 2) ** 2
        kernel = torch.where(t == 0, torch.ones_like(t), torch.sin(t) / t) * window
        kernel.div_(kernel.sum())
        rows.append(kernel)
    return torch.stack(rows), old, new, width


def taps64(old_sr, new_sr, zeros=24, rolloff=0.945):
    return taps_in(torch.float64, old_sr, new_sr, zeros, rolloff)


class ResampleFrac:
    """``julius.resample.ResampleFrac(old_sr, new_sr, zeros, rolloff)``: replicate padding by ``width`` and ``width +
    old``, ``F.conv1d(stride=old)`` with the ``new`` phases as output channels, a transpose, the first ``floor(new L /
    old)`` samples (in integers).  Over the last dimension."""

    def __init__(self, old_sr: int, new_sr: int, zeros: int = 24, rolloff: float = 0.945):
        self.taps, self.old, self.new, self.width = taps_in(torch.float32, old_sr, new_sr, zeros, rolloff)

    def padded(self, x: torch.Tensor) -> torch.Tensor:
        return F.pad(x.reshape(-1, 1, x.shape[-1]), (self.width, self.width + self.old), mode="replicate")

    def __call__(self, x: torch.Tensor) -> torch.Tensor:
        if self.old == self.new:
            return x
        length = x.shape[-1]
        ys = F.conv1d(self.padded(x), self.taps.to(x.dtype)[:, None], stride=self.old)
        y = ys.transpose(1, 2).reshape(list(x.shape[:-1]) + [-1])
        return y[..., :self.new * length // self.old]

    def magnitude(self, x: torch.Tensor) -> torch.Tensor:
        """``(|taps| conv |x|)[n]`` in fp64: what the summation bound of an output scales with."""
        length = x.shape[-1]
        ys = F.conv1d(self.padded(x.double().abs()), self.taps.double().abs()[:, None], stride=self.old)
        return ys.transpose(1, 2).reshape(list(x.shape[:-1]) + [-1])[..., :self.new * length // self.old]


def yin_direct(sig, sr=16_000, w_len=256, w_step=64, harmo_thresh=0.1, f0_min=100.0, f0_max=350.0):
    """``(pitches fp32 [frames], margin)``: the pitches of ``compute_yin`` with ``d(tau) = sum_j (x_j - x_{j + tau})^2``
    summed directly in fp64 (``j`` ascending), and the smallest ``|c - thresh|`` / ``|c(tau + 1) - c(tau)|`` of any
    comparison taken (``inf`` when every comparison involved a NaN)."""
    sig = np.asarray(sig, dtype=np.float64)
    tau_min, tau_max = int(sr / f0_max), int(sr / f0_min)
    starts = range(0, len(sig) - w_len, w_step)
    out = np.zeros(len(starts), dtype=np.float32)
    margin = math.inf
    with np.errstate(invalid="ignore", divide="ignore"):
        for n, t in enumerate(starts):
            x = sig[t:t + w_len]
            d = np.zeros(tau_max)
            for tau in range(1, tau_max):
                diff = x[:w_len - tau] - x[tau:]
                d[tau] = np.cumsum(diff * diff)[-1]             # one after the other, j ascending
            c = np.zeros(tau_max)
            csum = np.cumsum(d[1:])
            c[1:] = d[1:] * np.arange(1, tau_max) / csum
            if not np.isfinite(csum).all():
                c[1:] = np.nan                                  # the reference's FFT makes NaN of every lag
            tau, found = tau_min, 0
            while tau < tau_max:
                if not np.isnan(c[tau]):
                    margin = min(margin, abs(c[tau] - harmo_thresh))
                if c[tau] < harmo_thresh:
                    while tau + 1 < tau_max:
                        margin = min(margin, abs(c[tau + 1] - c[tau]))
                        if not c[tau + 1] < c[tau]:
                            break
                        tau += 1
                    found = tau
                    break
                tau += 1
            out[n] = np.float32(sr / found) if found else 0.0
    return out, margin


def pitch_signals():
    """The seeded signals of the fixture at 16 kHz: name -> fp32 [L]."""
    sr, L = 16_000, 16_000
    g = torch.Generator().manual_seed(1913)
    t = torch.arange(L, dtype=torch.float64) / sr
    f0 = 180.0 + 40.0 * torch.sin(2 * math.pi * 1.5 * t)                            # a vibrato between 140 and 220 Hz
    phase = 2 * math.pi * torch.cumsum(f0, 0) / sr
    tone = 0.5 * torch.sin(phase) + 0.2 * torch.sin(2 * phase + 0.7)
    voiced = (tone + 0.02 * torch.randn(L, generator=g, dtype=torch.float64)).float()
    mixed = voiced.clone()
    mixed[4000:7000] = 0.0                                                           # a silent stretch
    mixed[10000:13000] = 0.3 * torch.randn(3000, generator=g)                        # a pure-noise stretch
    out = dict(voiced=voiced, mixed=mixed)
    for name, n in (("len_w1", 257), ("len_ws", 320), ("len_ws1", 321)):             # w_len + 1, + w_step, + w_step + 1
        out[name] = voiced[2000:2000 + n].clone()
    return out


PITCH_PARAMS = {
    "default": dict(min_f0=100.0, max_f0=350.0, harmonic_thresh=0.1, frame_length_in_samples=256,
                    frame_space_in_samples=64),
    "wide": dict(min_f0=100.0, max_f0=500.0, harmonic_thresh=0.1, frame_length_in_samples=512,
                 frame_space_in_samples=256),
}


def yin_kwargs(params: dict) -> dict:
    """The keywords of ``hip_ops.yin_pitch`` / ``yin_direct`` for a ``Pitch`` parameter set."""
    return dict(w_len=params["frame_length_in_samples"], w_step=params["frame_space_in_samples"],
                harmo_thresh=params["harmonic_thresh"], f0_min=params["min_f0"], f0_max=params["max_f0"])


def stereo_441(L: int = 11_025, seed: int = 77) -> torch.Tensor:
    """The fixture's stereo waveform at 44.1 kHz: fp32 [2, L]."""
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L, dtype=torch.float64) / 44_100
    f0 = 160.0 + 25.0 * torch.sin(2 * math.pi * 2.0 * t)
    phase = 2 * math.pi * torch.cumsum(f0, 0) / 44_100
    tone = 0.4 * torch.sin(phase) + 0.15 * torch.sin(2 * phase + 0.3) + 0.05 * torch.sin(2 * math.pi * 3100.0 * t)
    noise = 0.02 * torch.randn(2, L, generator=g, dtype=torch.float64)
    return (tone[None] * torch.tensor([[1.0], [0.6]], dtype=torch.float64) + noise + 0.05).float()


_fixture = None


def fixture():
    """tests/golden/audio_rates.npz, read once: ``dict(meta=..., arrays)``."""
    global _fixture
    if _fixture is None:
        z = np.load(GOLDEN)
        _fixture = {k: z[k] for k in z.files}
        _fixture["meta"] = json.loads(str(z["meta"]))
    return _fixture
