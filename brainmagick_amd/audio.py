"""The MelSpectrum targets computed on the device from the waveform: bm/features/audio.py:31-83 (``MelSpectrum``) with
the sounds resident on the card and two launches for all of them (``hip_ops.mel_spectrograms``, csrc/mel.hip).

The reference computes one event's spectrogram on the CPU with ``torchaudio.transforms.MelSpectrogram`` and caches it on
disk.  torchaudio is not part of this stack, so the transform is restated from its documentation (``torch.stft`` with
``center=True``, reflect padding and a periodic Hann window, ``normalized`` = division by ``sqrt(sum w^2)``, ``|.|^2``,
the htk filterbank); see "Parity that cannot be pinned" in the README.  ``DeviceMelSpectrum.compute`` returns the
``[n_mels, L]`` arrays that ``DeviceEvents`` reads in place under the ``resampled`` rule.

Not built: julius' fractional resampling (a rate other than ``in_sampling`` raises), reading audio files, ``Pitch``,
wav2vec2 and the text embeddings, a backward pass (the targets are constants), and ``f_min`` / ``f_max`` / ``norm`` /
``mel_scale`` other than the reference's fixed choices.  There is no CPU fallback.
"""
import math
import typing as tp

import torch

from . import hip_ops as H
from .features import EventFeature


class DeviceMelSpectrum:
    """``MelSpectrum`` of the reference by its own names and defaults.  ``sample_rate`` is the rate of the features
    (the MEG's), ``in_sampling`` the rate the waveforms must have."""
    event_kind = "sound"

    def __init__(self, sample_rate: float, n_mels: int = 40, n_fft: int = 512, in_sampling: int = 16_000,
                 normalized: bool = True, use_log_scale: bool = True, log_scale_eps: float = 1e-5,
                 norm_audio: bool = True):
        H.mel_check_limits(n_fft, n_mels)
        if use_log_scale and not log_scale_eps > 0:
            raise ValueError(f"mel spectrogram: log_scale_eps = {log_scale_eps} under a logarithm")
        self.sample_rate = sample_rate
        self.dimension = n_mels
        self.in_sampling = in_sampling
        self.n_mels = n_mels
        self.n_fft = n_fft
        self.hop_length = n_fft // 4
        self.use_log_scale = use_log_scale
        self.log_scale_eps = log_scale_eps
        self.normalized = normalized
        self.norm_audio = norm_audio
        self.default_value = math.log10(log_scale_eps) if use_log_scale else 0.0       # audio.py:58-59, base.py's 0.

    def feature(self, name: str = "MelSpectrum") -> EventFeature:
        """The entry of a ``DeviceFeaturesBuilder`` that paints the arrays of ``compute``."""
        return EventFeature(name, "resampled", self.event_kind, self.n_mels, default_value=self.default_value)

    def compute(self, wavs: tp.Sequence[torch.Tensor],
                sample_rates: tp.Union[float, tp.Sequence[float]]) -> tp.List[torch.Tensor]:
        """One ``[n_mels, 1 + L // hop_length]`` fp32 device tensor per sound.  ``wavs``: ``[L]`` or ``[channels, L]``
        fp32 device tensors (the channel mean is a torch op); ``sample_rates``: one rate for all, or one per sound."""
        wavs = list(wavs)
        rates = list(sample_rates) if isinstance(sample_rates, (list, tuple)) else [sample_rates] * len(wavs)
        if len(rates) != len(wavs):
            raise ValueError(f"mel spectrogram: {len(wavs)} waveforms and {len(rates)} sample rates")
        mono = []
        for i, (wav, sr) in enumerate(zip(wavs, rates)):
            if int(sr) != int(self.in_sampling) or float(sr) != float(int(sr)):
                raise ValueError(f"mel spectrogram: sound {i} is sampled at {sr} Hz; resampling to in_sampling = "
                                 f"{self.in_sampling} Hz is not built")
            if not isinstance(wav, torch.Tensor) or wav.dim() not in (1, 2):
                raise ValueError(f"mel spectrogram: sound {i} is not a [L] or [channels, L] tensor")
            mono.append(wav if wav.dim() == 1 else torch.mean(wav, dim=0))
        return H.mel_spectrograms(mono, self.n_mels, self.n_fft, self.in_sampling, self.normalized, self.use_log_scale,
                                  self.log_scale_eps, self.norm_audio)
