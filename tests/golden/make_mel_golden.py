"""Golden vectors of the MelSpectrum feature, from the REAL reference ``MelSpectrum.__init__`` / ``_compute``
(bm/features/audio.py:31-76, read-only /root/reference).

Run in the build container only:   python tests/golden/make_mel_golden.py [output directory]
Writes ``mel_spectrum.npz`` (default: next to this file).

The reference runs under stubs, as in make_features_golden.py (``_ref_import.py`` is not touched): ``bm`` and
``bm.features`` are skeleton packages, ``bm.cache`` is a pass-through (the cache is bypassed), ``bm.utils``,
``bm.events``, ``bm.features.base`` and ``bm.features.audio`` are the reference's own files, unmodified.  Three names in
``audio``'s scope are stand-ins, because what they name cannot run here:

- ``torchaudio.transforms.MelSpectrogram`` RESTATES torchaudio's documented transform with ``torch.stft``
  (tests/mel_cases.py: ``stft_mel``), in the dtype of the waveform it is handed;
- ``julius.resample.ResampleFrac(old_sr, new_sr)`` asserts equal rates and returns its input;
- ``_extract_wav_part`` returns the case's seeded stereo waveform at 16 kHz.

So the fixture pins the WIRING to the live reference -- the channel mean, the normalisation with the unbiased std and
its 1e-8, ``hop_length = n_fft // 4``, the order of transform and logarithm, the eps, ``default_value`` -- and the
transform to the restatement.  Per case: the output of ``_compute`` on the fp32 waveform (``out32``) and of the same code
on the waveform in fp64 (``out64``).  Cases (``wave_a``: 1000 samples, ``wave_b``: 4000 samples, both stereo):

  ``ref_test``      n_fft 100, n_mels 8, L 1000: the parameters of the reference's own test
  ``silence_120``   n_fft 512, n_mels 120, L 4000, samples [1650, 2350) zero: an all-zero filter, silent frames
  ``no_norm_audio`` / ``no_log`` / ``no_normalized``   n_fft 512, n_mels 40, L 4000, one switch off each

This file holds none of the reference's text.
"""
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
REF = Path("/root/reference")

import mel_cases as MC  # noqa: E402

IN_SAMPLING = 16_000
CASES = [
    dict(name="ref_test", n_fft=100, n_mels=8, L=1000, wave="wave_a", silence=None, kw={}),
    dict(name="silence_120", n_fft=512, n_mels=120, L=4000, wave="wave_b", silence=[1650, 2350], kw={}),
    dict(name="no_norm_audio", n_fft=512, n_mels=40, L=4000, wave="wave_b", silence=None, kw=dict(norm_audio=False)),
    dict(name="no_log", n_fft=512, n_mels=40, L=4000, wave="wave_b", silence=None, kw=dict(use_log_scale=False)),
    dict(name="no_normalized", n_fft=512, n_mels=40, L=4000, wave="wave_b", silence=None, kw=dict(normalized=False)),
]
_current = {}               # what ``_extract_wav_part`` hands out


class RestatedMelSpectrogram:
    def __init__(self, sample_rate, n_mels, n_fft, hop_length, normalized):
        assert hop_length == n_fft // 4
        self.args = (n_fft, n_mels, sample_rate, normalized)

    def __call__(self, wav):
        return MC.stft_mel(wav, *self.args)


class SameRate:
    def __init__(self, old_sr, new_sr):
        assert old_sr == new_sr, (old_sr, new_sr)

    def __call__(self, wav):
        return wav


def load_reference():
    if not REF.exists():
        raise RuntimeError("/root/reference not available: the fixture can only be regenerated in the build container")

    def stub(name, **attrs):
        mod = types.ModuleType(name)
        mod.__dict__.update(attrs)
        sys.modules[name] = mod
        return mod

    class PassThrough:
        def __init__(self, *args, **kwargs):
            pass

        def get(self, _computation, *args, **kwargs):
            return _computation(*args, **kwargs)

    stub("mne")
    stub("transformers")
    stub("julius", resample=types.SimpleNamespace(ResampleFrac=SameRate))
    stub("torchaudio", transforms=types.SimpleNamespace(MelSpectrogram=RestatedMelSpectrogram), info=None)
    stub("dora", to_absolute_path=lambda p: p, log=stub("dora.log", LogProgress=object))
    stub("omegaconf", OmegaConf=object, basecontainer=stub("omegaconf.basecontainer", BaseContainer=object))
    bm = stub("bm")
    bm.__path__ = [str(REF / "bm")]                  # submodules are found, bm/__init__.py does not run
    stub("bm.cache", Cache=PassThrough, MemoryCache=PassThrough)
    stub("bm.lib.pitch_calc")
    stub("bm.lib.pitch_calc.yin", compute_yin=None)
    feats = stub("bm.features")
    feats.__path__ = [str(REF / "bm" / "features")]
    import importlib
    audio = importlib.import_module("bm.features.audio")
    utils = importlib.import_module("bm.utils")
    audio._extract_wav_part = lambda filepath, start, stop: (_current["wav"], IN_SAMPLING)
    return audio, utils


def make_waves():
    g = torch.Generator().manual_seed(4212)
    waves = {}
    for key, L in (("wave_a", 1000), ("wave_b", 4000)):
        t = torch.arange(L) / IN_SAMPLING
        tone = 0.3 * torch.sin(2 * torch.pi * 440.0 * t) + 0.1 * torch.sin(2 * torch.pi * 3100.0 * t)
        noise = 0.2 * torch.randn(2, L, generator=g)
        waves[key] = (tone[None] * torch.tensor([[1.0], [0.6]]) + noise + 0.05).float().numpy()
    return waves


def build() -> dict:
    torch.set_num_threads(1)          # the reference's CPU reductions in one fixed order: regeneration is bit-exact
    audio, utils = load_reference()
    waves = make_waves()
    out = dict(waves)
    meta = []
    for case in CASES:
        wave = waves[case["wave"]].copy()
        if case["silence"]:
            wave[:, case["silence"][0]:case["silence"][1]] = 0.0
        feature = audio.MelSpectrum(sample_rate=utils.Frequency(120.0), n_mels=case["n_mels"], n_fft=case["n_fft"],
                                    in_sampling=IN_SAMPLING, **case["kw"])
        for dtype, key in ((torch.float32, "out32"), (torch.float64, "out64")):
            _current["wav"] = torch.from_numpy(wave).to(dtype)
            res = feature._compute(Path("never_opened.wav"), 0.0, case["L"] / IN_SAMPLING)
            assert res.dtype == dtype and res.shape == (case["n_mels"], 1 + case["L"] // (case["n_fft"] // 4)), res.shape
            out[f"{case['name']}/{key}"] = res.numpy().copy()
        meta.append(dict(name=case["name"], n_fft=case["n_fft"], n_mels=case["n_mels"], L=case["L"], wave=case["wave"],
                         silence=case["silence"], in_sampling=IN_SAMPLING, norm_audio=feature.norm_audio,
                         use_log_scale=feature.use_log_scale, normalized=feature.normalized,
                         log_scale_eps=feature.log_scale_eps,
                         attributes=dict(dimension=feature.dimension, default_value=float(feature.default_value),
                                         hop_length=feature.hop_length, event_kind=feature.event_kind,
                                         n_mels=feature.n_mels, n_fft=feature.n_fft, in_sampling=feature.in_sampling)))
    out["meta"] = json.dumps(dict(cases=meta, torch=torch.__version__))
    return out


def main(argv):
    dest = Path(argv[0]) if argv else HERE
    dest.mkdir(parents=True, exist_ok=True)
    out = build()
    np.savez_compressed(dest / "mel_spectrum.npz", **out)
    size = (dest / "mel_spectrum.npz").stat().st_size
    assert size < 200_000, size
    print(f"mel_spectrum: {len(out)} arrays -> {dest / 'mel_spectrum.npz'} ({size} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
