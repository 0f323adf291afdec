"""Golden vectors of the Pitch feature and of the resampling in front of both audio features, from the REAL reference
``Pitch._compute`` / ``MelSpectrum._compute`` (bm/features/audio.py:61-76, 110-124) and ``compute_yin``
(bm/lib/pitch_calc/yin.py), read-only /root/reference.

Run in the build container only:   python tests/golden/make_audio_rates_golden.py [output directory]
Writes ``audio_rates.npz`` (default: next to this file).

The reference runs under the stubs of make_mel_golden.py, with three differences:

- ``bm.lib.pitch_calc.yin`` is the reference's own file, imported under a stand-in ``numba`` (``jit`` and ``overload``
  as identity decorators, ``objmode`` as a null context manager): it then runs as plain numpy;
- ``julius.resample.ResampleFrac`` is the restatement of tests/audio_cases.py (julius' published definition in torch
  ops, in the dtype of the waveform it is handed);
- ``_extract_wav_part`` hands out the case's waveform AND its rate.

So the fixture pins YIN to the live reference, and the order of channel mean, normalisation, resampling and transform
and the output lengths to the live ``_compute``; the resampler and the mel transform are the restatements.

Pitch cases (16 kHz, no resampling): the signals of ``audio_cases.pitch_signals`` under both parameter sets of
``audio_cases.PITCH_PARAMS``.  For every frame the maker also evaluates the direct form of the difference function
(``audio_cases.yin_direct``) and asserts that it gives the same pitches and that no comparison it took was closer than
1e-9 (the FFT and the direct form differ near 1e-13): equality tests are legitimate on these inputs.

Wiring cases (a stereo 44.1 kHz waveform of 11 025 samples): ``MelSpectrum._compute`` at (n_fft, n_mels) = (512, 40) and
(100, 8) and ``Pitch._compute``, on the waveform in fp32 (``out32``) and in fp64 (``out64``).

This file holds none of the reference's text.
"""
import contextlib
import json
import sys
import types
from pathlib import Path

import numpy as np
import torch

HERE = Path(__file__).resolve().parent
sys.path.insert(0, str(HERE.parent))
REF = Path("/root/reference")

import audio_cases as AC  # noqa: E402
import make_mel_golden as MM  # noqa: E402

MARGIN = 1e-9
MEL_WIRING = [dict(name="mel_512", n_fft=512, n_mels=40), dict(name="mel_100", n_fft=100, n_mels=8)]
_current = {}               # what ``_extract_wav_part`` hands out: wav, sr


def load_reference():
    def identity_decorator(*args, **kwargs):
        if len(args) == 1 and callable(args[0]) and not kwargs:
            return args[0]                              # @jit
        return lambda fn: fn                            # @jit(nopython=True)

    audio, utils = MM.load_reference()                  # its stubs; then the three differences
    numba = types.ModuleType("numba")
    numba.jit = identity_decorator
    numba.objmode = lambda **kw: contextlib.nullcontext()
    numba.types = types.SimpleNamespace(Array=())
    extending = types.ModuleType("numba.extending")
    extending.overload = lambda target: (lambda fn: fn)
    numba.extending = extending
    sys.modules["numba"], sys.modules["numba.extending"] = numba, extending
    import importlib.util
    spec = importlib.util.spec_from_file_location("bm_ref_yin", REF / "bm" / "lib" / "pitch_calc" / "yin.py")
    yin = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(yin)
    audio.compute_yin = yin.compute_yin
    audio.julius = types.SimpleNamespace(resample=types.SimpleNamespace(ResampleFrac=AC.ResampleFrac))
    audio._extract_wav_part = lambda filepath, start, stop: (_current["wav"], _current["sr"])
    return audio, utils, yin


def build() -> dict:
    torch.set_num_threads(1)          # the reference's CPU reductions in one fixed order: regeneration is bit-exact
    audio, utils, yin = load_reference()
    out, meta = {}, dict(pitch=[], wiring=[], torch=torch.__version__, numpy=np.__version__)
    smallest, frames, voiced = float("inf"), 0, 0

    signals = AC.pitch_signals()
    for name, sig in signals.items():
        out[f"signal/{name}"] = sig.numpy().copy()
    for pname, params in AC.PITCH_PARAMS.items():
        feature = audio.Pitch(sample_rate=utils.Frequency(120.0), **params)
        assert feature.in_sampling == 16_000
        for name, sig in signals.items():
            if sig.numel() <= params["frame_length_in_samples"]:
                continue                                # the boundary lengths belong to the default frame length
            _current.update(wav=sig[None], sr=utils.Frequency(16_000))
            res = feature._compute(Path("never_opened.wav"), 0.0, sig.numel() / 16_000)
            assert res.dtype == torch.float32 and res.dim() == 1
            kw = AC.yin_kwargs(params)
            live = yin.compute_yin(sig.numpy(), 16_000, kw["w_len"], kw["w_step"], kw["f0_min"], kw["f0_max"],
                                   kw["harmo_thresh"])[0]
            assert np.array_equal(res.numpy(), np.asarray(live, dtype=np.float32))
            direct, margin = AC.yin_direct(sig.numpy(), 16_000, **kw)
            assert np.array_equal(direct, res.numpy()), (pname, name)
            assert margin >= MARGIN, (pname, name, margin)
            smallest, frames, voiced = min(smallest, margin), frames + len(direct), voiced + int((direct > 0).sum())
            out[f"pitch/{pname}/{name}"] = res.numpy().copy()
            meta["pitch"].append(dict(params=pname, signal=name, frames=len(direct), margin=margin))

    stereo = AC.stereo_441()
    out["wiring/wave"] = stereo.numpy().copy()
    L, sr = stereo.shape[1], 44_100
    for case in MEL_WIRING:
        feature = audio.MelSpectrum(sample_rate=utils.Frequency(120.0), n_mels=case["n_mels"], n_fft=case["n_fft"])
        for dtype, key in ((torch.float32, "out32"), (torch.float64, "out64")):
            _current.update(wav=stereo.to(dtype), sr=utils.Frequency(sr))
            res = feature._compute(Path("never_opened.wav"), 0.0, L / sr)
            n16 = 16_000 * L // sr
            assert res.dtype == dtype and res.shape == (case["n_mels"], 1 + n16 // (case["n_fft"] // 4)), res.shape
            out[f"wiring/{case['name']}/{key}"] = res.numpy().copy()
        meta["wiring"].append(dict(case, kind="mel", sr=sr, L=L, in_sampling=feature.in_sampling,
                                   norm_audio=feature.norm_audio, use_log_scale=feature.use_log_scale,
                                   normalized=feature.normalized, log_scale_eps=feature.log_scale_eps))
    feature = audio.Pitch(sample_rate=utils.Frequency(120.0))
    kw = AC.yin_kwargs(AC.PITCH_PARAMS["default"])
    for dtype, key in ((torch.float32, "out32"), (torch.float64, "out64")):
        _current.update(wav=stereo.to(dtype), sr=utils.Frequency(sr))
        res = feature._compute(Path("never_opened.wav"), 0.0, L / sr)
        at16 = AC.ResampleFrac(sr, 16_000)(torch.mean(stereo.to(dtype), dim=0))
        direct, margin = AC.yin_direct(at16.numpy(), 16_000, **kw)
        assert res.dtype == torch.float32 and np.array_equal(direct, res.numpy()) and margin >= MARGIN, margin
        smallest, frames, voiced = min(smallest, margin), frames + len(direct), voiced + int((direct > 0).sum())
        out[f"wiring/pitch/{key}"] = res.numpy().copy()
    meta["wiring"].append(dict(name="pitch", kind="pitch", sr=sr, L=L, in_sampling=16_000))
    meta.update(smallest_margin=smallest, frames=frames, voiced=voiced)
    print(f"audio_rates: smallest margin of any comparison {smallest:.2e} over {frames} frames, {voiced} voiced")
    out["meta"] = json.dumps(meta)
    return out


def main(argv):
    dest = Path(argv[0]) if argv else HERE
    dest.mkdir(parents=True, exist_ok=True)
    out = build()
    np.savez_compressed(dest / "audio_rates.npz", **out)
    size = (dest / "audio_rates.npz").stat().st_size
    assert size < 400_000, size
    print(f"audio_rates: {len(out)} arrays -> {dest / 'audio_rates.npz'} ({size} bytes)")


if __name__ == "__main__":
    main(sys.argv[1:])
