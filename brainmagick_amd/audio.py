"""The audio features computed on the device from the waveform: bm/features/audio.py:31-132 (``MelSpectrum``, ``Pitch``)
with the sounds resident on the card and a few launches for all of them (``hip_ops.mel_spectrograms``, csrc/mel.hip;
``hip_ops.resample_frac``, csrc/resample.hip; ``hip_ops.yin_pitch``, csrc/pitch.hip).

The reference computes one event's feature on the CPU -- ``julius.resample.ResampleFrac`` to 16 kHz, then
``torchaudio.transforms.MelSpectrogram`` or ``compute_yin`` -- and caches it on disk.  torchaudio and julius are not part
of this stack, so both are restated from their published definitions (``torch.stft`` with ``center=True``, reflect
padding and a periodic Hann window, ``normalized`` = division by ``sqrt(sum w^2)``, ``|.|^2``, the htk filterbank; a
polyphase filter of Hann-windowed sincs); see "Parity that cannot be pinned" in the README.  ``compute`` returns the
``[dimension, L]`` arrays that ``DeviceEvents`` reads in place under the ``resampled`` rule.

The resampler cannot be held to julius here, so ``compute`` resamples only when asked (``resample=True``); without the
switch a rate other than ``in_sampling`` raises.

Not built: reading audio files, wav2vec2 and the text embeddings, a backward pass (the targets are constants),
non-integer sample rates, and ``f_min`` / ``f_max`` / ``norm`` / ``mel_scale`` other than the reference's fixed choices.
There is no CPU fallback.
"""
import math
import typing as tp

import torch

from . import hip_ops as H
from .features import EventFeature


def _mono_at_rates(what: str, wavs, sample_rates, in_sampling: int, resample: bool):
    """``(mono waveforms, integer rates)`` behind the checks that both features share."""
    wavs = list(wavs)
    rates = list(sample_rates) if isinstance(sample_rates, (list, tuple)) else [sample_rates] * len(wavs)
    if len(rates) != len(wavs):
        raise ValueError(f"{what}: {len(wavs)} waveforms and {len(rates)} sample rates")
    mono = []
    for i, (wav, sr) in enumerate(zip(wavs, rates)):
        if float(sr) != float(int(sr)) or int(sr) < 1:
            raise ValueError(f"{what}: sound {i} is sampled at {sr} Hz; resampling from a rate that is not a positive "
                             "integer is not built")
        if int(sr) != int(in_sampling) and not resample:
            raise ValueError(f"{what}: sound {i} is sampled at {sr} Hz; resampling to in_sampling = {in_sampling} Hz is a "
                             "restatement of julius' filter that cannot be held to it: pass resample=True")
        if not isinstance(wav, torch.Tensor) or wav.dim() not in (1, 2):
            raise ValueError(f"{what}: sound {i} is not a [L] or [channels, L] tensor")
        mono.append(wav if wav.dim() == 1 else torch.mean(wav, dim=0))
    return mono, [int(sr) for sr in rates]


def _resample_all(mono, rates, in_sampling: int, moments: tp.Optional[torch.Tensor]):
    """``mono`` with every sound at another rate replaced by its resampled form: one ``bm_resample_frac`` per distinct
    reduced ratio (in the order of first appearance), normalising on the way when ``moments`` are given."""
    groups: tp.Dict[tp.Tuple[int, int], tp.List[int]] = {}
    for i, sr in enumerate(rates):
        if sr != int(in_sampling):
            groups.setdefault(H.resample_ratio(sr, int(in_sampling)), []).append(i)
    out = list(mono)
    for (old, new), idx in groups.items():
        mom = None
        if moments is not None:
            mom = moments[torch.tensor(idx, device=moments.device)] if len(idx) != len(mono) else moments
        for i, wav in zip(idx, H.resample_frac([mono[i] for i in idx], old, new, moments=mom)):
            out[i] = wav
    return out


class DeviceMelSpectrum:
    """``MelSpectrum`` of the reference by its own names and defaults.  ``sample_rate`` is the rate of the features
    (the MEG's), ``in_sampling`` the rate the transform works at."""
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

    def compute(self, wavs: tp.Sequence[torch.Tensor], sample_rates: tp.Union[float, tp.Sequence[float]],
                resample: bool = False) -> tp.List[torch.Tensor]:
        """One ``[n_mels, 1 + L // hop_length]`` fp32 device tensor per sound, ``L`` its length at ``in_sampling``.
        ``wavs``: ``[L]`` or ``[channels, L]`` fp32 device tensors (the channel mean is a torch op); ``sample_rates``:
        one rate for all, or one per sound.  A sound at another (integer) rate raises unless ``resample=True``.

        Launches for the whole call: ``bm_wave_moments`` (with ``norm_audio``) and ``bm_mel_spectrogram`` when every
        sound is at ``in_sampling`` -- today's two, and today's bits for those sounds in any call; otherwise
        ``bm_wave_moments`` of the SOURCE waveforms (with ``norm_audio``: the reference normalises before it
        resamples), one ``bm_resample_frac`` per distinct reduced ratio, which normalises on the way, and
        ``bm_mel_spectrogram`` with identity moments for the resampled sounds: ``2 + ratios`` launches, ``1 + ratios``
        without ``norm_audio``."""
        mono, rates = _mono_at_rates("mel spectrogram", wavs, sample_rates, self.in_sampling, resample)
        args = (self.n_mels, self.n_fft, self.in_sampling, self.normalized, self.use_log_scale, self.log_scale_eps)
        other = [sr != int(self.in_sampling) for sr in rates]
        if not any(other):
            return H.mel_spectrograms(mono, *args, self.norm_audio)
        if not self.norm_audio:
            return H.mel_spectrograms(_resample_all(mono, rates, self.in_sampling, None), *args, False)
        moments = H.wave_moments(mono)
        at_rate = _resample_all(mono, rates, self.in_sampling, moments)
        identity = torch.tensor([0.0, 1.0], dtype=torch.float64, device=moments.device)
        moments = torch.where(torch.tensor(other, device=moments.device)[:, None], identity, moments)
        return H.mel_spectrograms(at_rate, *args, True, moments=moments)


class DevicePitch:
    """``Pitch`` of the reference by its own names and defaults: YIN on the channel mean at 16 kHz, no normalisation of
    the audio.  ``sample_rate`` is the rate of the features (the MEG's)."""
    event_kind = "sound"
    dimension = 1
    default_value = 0.0

    def __init__(self, sample_rate: float, min_f0: float = 100.0, max_f0: float = 350.0, harmonic_thresh: float = 0.1,
                 frame_length_in_samples: int = 256, frame_space_in_samples: int = 64):
        self.sample_rate = sample_rate
        self.frame_length_in_samples = frame_length_in_samples
        self.frame_space_in_samples = frame_space_in_samples
        self.harmonic_thresh = harmonic_thresh
        self.min_f0 = min_f0
        self.max_f0 = max_f0
        self.in_sampling = 16_000
        H.yin_taus(self.in_sampling, frame_length_in_samples, frame_space_in_samples, min_f0, max_f0)

    def feature(self, name: str = "Pitch") -> EventFeature:
        """The entry of a ``DeviceFeaturesBuilder`` that paints the arrays of ``compute``."""
        return EventFeature(name, "resampled", self.event_kind, self.dimension, default_value=self.default_value)

    def compute(self, wavs: tp.Sequence[torch.Tensor], sample_rates: tp.Union[float, tp.Sequence[float]],
                resample: bool = False) -> tp.List[torch.Tensor]:
        """One ``[1, len(range(0, L - frame_length, frame_space))]`` fp32 device tensor per sound, ``L`` its length at
        16 kHz.  ``wavs`` and ``sample_rates`` as for ``DeviceMelSpectrum.compute``; a sound at another rate raises
        unless ``resample=True``.  Launches: one ``bm_resample_frac`` per distinct reduced ratio, one ``bm_yin_pitch``."""
        mono, rates = _mono_at_rates("pitch", wavs, sample_rates, self.in_sampling, resample)
        if any(sr != self.in_sampling for sr in rates):
            mono = _resample_all(mono, rates, self.in_sampling, None)
        return H.yin_pitch(mono, self.in_sampling, self.frame_length_in_samples, self.frame_space_in_samples,
                           self.harmonic_thresh, self.min_f0, self.max_f0)
