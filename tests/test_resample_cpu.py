"""The host side of the resampler without a GPU: ``hip_ops.resample_taps`` against the fp64 restatement of
tests/audio_cases.py, the table's shapes, the restated ``ResampleFrac`` on a sine, the fixture's wiring cases
(tests/golden/make_audio_rates_golden.py: the live reference's ``_compute`` around the restatements), every limit, the
declared entry points and the ISA of csrc/resample.hip.  Reads the fixture only."""
import math
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

import audio_cases as AC
import mel_cases as MC

RATIOS = [(44_100, 16_000, 441, 160, 70, 581), (48_000, 16_000, 3, 1, 77, 157), (8_000, 16_000, 1, 2, 26, 53),
          (32_000, 16_000, 2, 1, 51, 104), (24_000, 16_000, 3, 2, 39, 81), (22_050, 16_000, 441, 320, 35, 511),
          (11_025, 16_000, 441, 640, 26, 493)]


def _taps_tol(old, new, width, zeros, rolloff):
    sr = min(old, new) * rolloff
    arg_err = 2.0 ** -24 * (2 * (width + old) / old * sr * math.pi + 3 * zeros * math.pi)
    return 4 * arg_err + 8 * 2.0 ** -24


@pytest.mark.parametrize("old_sr,new_sr,old,new,width,ntaps", RATIOS)
def test_taps_against_the_fp64_restatement(old_sr, new_sr, old, new, width, ntaps):
    """The bound, from the fp32 expressions alone.  The argument of a tap is ``t = (-i / new + idx / old) * sr * pi``:
    the two terms of the sum (at most ``m = (width + old) / old`` in size) are rounded before they cancel, which ``sr *
    pi`` then magnifies, and the three products behind it are relative roundings of ``|t| <= zeros * pi``:
    ``arg_err = 2^-24 (2 m sr pi + 3 zeros pi)``.  The slope of ``sinc * window`` is below ``min(0.5, 1.1 / |t|)``: a tap
    is off by ``0.5 arg_err`` at most before the division by the phase's sum ``S = old / sr > 1``, and that sum by at
    most ``arg_err`` times the sum of the slopes over taps ``pi / S`` apart, ``(2 S / pi) (1.1 + 1.1 ln(zeros pi /
    2.2)) = 3.2 S`` -- a relative 3.2 ``arg_err`` on taps below ``1 / S``.  Together under ``4 arg_err``, plus eight
    roundings of values below 1 (sin, the quotient, the window, the division)."""
    from brainmagick_amd import hip_ops as H
    taps, o, n, w = H.resample_taps(old_sr, new_sr)
    assert (o, n, w) == (old, new, width) and taps.dtype == torch.float32 and tuple(taps.shape) == (new, ntaps)
    assert ntaps == 2 * width + old
    want = AC.taps64(old_sr, new_sr)[0]
    err = float((taps.double() - want).abs().max())
    tol = _taps_tol(old, new, width, 24, 0.945)
    print(f"taps {old}/{new}: largest deviation from fp64 {err:.2e}, bound {tol:.2e}")
    assert err <= tol
    assert float((taps.double().sum(1) - 1).abs().max()) <= ntaps * 2.0 ** -24      # a sum of ntaps fp32 values of sum 1
    assert torch.equal(taps, AC.ResampleFrac(old_sr, new_sr).taps)                  # the fp32 expressions themselves
    assert H.resample_taps(old_sr, new_sr)[0] is taps                               # cached
    assert H.resample_taps(old_sr // 5, new_sr // 5)[0] is taps                     # ... per reduced ratio


def test_other_zeros_and_rolloff():
    from brainmagick_amd import hip_ops as H
    taps, old, new, width = H.resample_taps(3, 2, zeros=8, rolloff=0.8)
    assert (old, new, width) == (3, 2, math.ceil(8 * 3 / 1.6)) and tuple(taps.shape) == (2, 2 * width + 3)
    assert float((taps.double() - AC.taps64(3, 2, 8, 0.8)[0]).abs().max()) <= _taps_tol(3, 2, width, 8, 0.8)


def test_a_sine_comes_out_as_the_same_sine():
    """1 kHz at 44.1 kHz -> 1 kHz at 16 kHz, sample n at time n / 16000; the restatement is within 2e-5 of it in the
    interior here; the bound is the issue's."""
    L = 44_100 // 4
    x = torch.sin(2 * math.pi * 1000.0 * torch.arange(L, dtype=torch.float64) / 44_100).float()
    y = AC.ResampleFrac(44_100, 16_000)(x)
    assert y.shape == (16_000 * L // 44_100,) and y.dtype == torch.float32
    want = torch.sin(2 * math.pi * 1000.0 * torch.arange(y.numel(), dtype=torch.float64) / 16_000)
    inner = slice(100, y.numel() - 100)
    err = float((y.double()[inner] - want[inner]).abs().max())
    print(f"1 kHz sine 44.1 -> 16 kHz: {err:.2e} from the sine in the interior")
    assert err <= 2e-3


def test_output_lengths_are_integer_floors():
    from brainmagick_amd import hip_ops as H
    for L in (1, 2, 440, 441, 442, 882, 11_025, 2 ** 31 - 1):
        assert H.resample_length(L, 441, 160) == (160 * L) // 441
    assert H.resample_length(3 * 2 ** 24 + 1, 3, 1) == 2 ** 24                     # where an fp32 quotient rounds up
    x = torch.zeros(1000)
    assert AC.ResampleFrac(3, 2)(x).shape == (666,) and AC.ResampleFrac(1, 2)(x).shape == (2000,)
    assert AC.ResampleFrac(16_000, 16_000)(x) is x


def _mel_chain(stereo, dtype, case):
    wav = torch.mean(stereo.to(dtype), dim=0)
    if case["norm_audio"]:
        wav = (wav - wav.mean()) / (1e-8 + wav.std())
    wav = AC.ResampleFrac(case["sr"], case["in_sampling"])(wav)
    mel = MC.stft_mel(wav, case["n_fft"], case["n_mels"], case["in_sampling"], case["normalized"])
    return MC.finish(mel, case["use_log_scale"], case["log_scale_eps"])


def test_fixture_is_the_wiring_around_the_restatements():
    """mean over channels -> normalisation -> resampling -> transform -> log in both precisions, the same torch ops in
    the order the live reference's ``_compute`` recorded: equal up to the order of the CPU's reductions."""
    fx = AC.fixture()
    stereo = torch.from_numpy(fx["wiring/wave"])
    for case in fx["meta"]["wiring"]:
        if case["kind"] != "mel":
            continue
        n16 = case["in_sampling"] * case["L"] // case["sr"]
        for dtype, key in ((torch.float32, "out32"), (torch.float64, "out64")):
            want = torch.from_numpy(fx[f"wiring/{case['name']}/{key}"])
            got = _mel_chain(stereo, dtype, case)
            assert got.shape == want.shape == (case["n_mels"], 1 + n16 // (case["n_fft"] // 4))
            assert torch.allclose(got, want, rtol=1e-5 if dtype == torch.float32 else 1e-12, atol=1e-6)
        # normalising AFTER the resampler is another function: the fixture tells the two orders apart
        wav = AC.ResampleFrac(case["sr"], case["in_sampling"])(torch.mean(stereo.double(), dim=0))
        wav = (wav - wav.mean()) / (1e-8 + wav.std())
        other = MC.finish(MC.stft_mel(wav, case["n_fft"], case["n_mels"], case["in_sampling"], case["normalized"]),
                          case["use_log_scale"], case["log_scale_eps"])
        assert float((other - torch.from_numpy(fx[f"wiring/{case['name']}/out64"])).abs().max()) > 1e-6


def test_every_limit_raises_its_value_error():
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.audio import DeviceMelSpectrum, DevicePitch
    wave = torch.zeros(4000)
    with pytest.raises(ValueError, match="identity"):
        H.resample_taps(16_000, 16_000)
    with pytest.raises(ValueError, match="integers"):
        H.resample_frac([wave], 44_100.5, 16_000)
    with pytest.raises(ValueError, match="integers"):
        H.resample_frac([wave], 0, 16_000)
    with pytest.raises(ValueError, match="at most 4096"):
        H.resample_frac([wave], 1, 4097)                                 # phases
    with pytest.raises(ValueError, match="at most 16384"):
        H.resample_frac([wave], 1100, 1099)                              # 15 old + ntaps floats of LDS
    assert H.resample_taps(44_100, 800)[0].shape == (8, 3241)            # 441 / 8 with 3241 taps: inside
    with pytest.raises(ValueError, match="zeros"):
        H.resample_frac([wave], 3, 2, zeros=0)
    with pytest.raises(ValueError, match="rolloff"):
        H.resample_frac([wave], 3, 2, rolloff=1.5)
    with pytest.raises(ValueError, match=r"2\^31"):
        H.resample_frac([torch.empty(2 ** 31, device="meta")], 3, 2)
    with pytest.raises(ValueError, match=r"fewer than 2\^31"):
        H.resample_frac([torch.empty(2 ** 30, device="meta")], 1, 2)     # the outputs
    with pytest.raises(ValueError, match="limit is 65535"):
        H.resample_frac([wave] * 65536, 3, 2)
    for old_sr in (44_100, 48_000, 32_000, 24_000, 22_050, 11_025, 8_000):          # the rates of the studies: inside
        assert H.resample_frames_tile(old_sr, 16_000) >= 16 and H.resample_frames_tile(old_sr, 16_000) % 16 == 0
        with pytest.raises(RuntimeError):                                # within the limits: no CPU fallback
            H.resample_frac([wave], old_sr, 16_000)
    for feature in (DeviceMelSpectrum(120.0), DevicePitch(120.0)):
        with pytest.raises(ValueError, match="resampling.*resample=True"):
            feature.compute([wave], 44_100)                              # the caller opts in
        with pytest.raises(ValueError, match="resampling"):
            feature.compute([wave], 44_100.5, resample=True)
        with pytest.raises(ValueError, match="sample rates"):
            feature.compute([wave, wave], [44_100], resample=True)
        with pytest.raises(RuntimeError):
            feature.compute([wave], 44_100, resample=True)


def test_frames_per_tile_are_a_function_of_the_ratio():
    from brainmagick_amd import hip_ops as H
    assert H.resample_frames_tile(44_100, 16_000) == 16 and H.resample_frames_tile(600, 599) == 16       # one MFMA row block
    assert H.resample_frames_tile(48_000, 16_000) == 1024 and H.resample_frames_tile(8_000, 16_000) == 1024
    assert H.resample_frames_tile(3, 32) == 16
    assert H.lib().bm_resample_frames_tile(1100, 1099, 26) == 0 and H.lib().bm_resample_frames_tile(1, 4097, 26) == 0


def test_library_declares_the_resample_entry_points():
    from brainmagick_amd import _lib
    from brainmagick_amd import hip_ops as H
    L = _lib.lib()
    assert L.bm_version() >= 115
    protos = _lib.parse_header()
    assert {"bm_resample_frac", "bm_resample_frames_tile"} <= set(protos)
    assert protos["bm_resample_frac"][2] == ["table", "lengths", "n_waves", "mom", "taps", "old_rate", "new_rate", "width",
                                             "stream"]
    for name in ("resample_frac", "resample_taps", "resample_length", "resample_frames_tile"):
        assert callable(getattr(H, name)), name
    import inspect
    sig = inspect.signature(H.resample_frac)
    assert {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == \
        dict(zeros=24, rolloff=0.945, moments=None)
    sig = inspect.signature(H.mel_spectrograms)
    assert sig.parameters["moments"].default is None


def test_resample_kernels_use_no_scratch_and_the_exact_fp32_mfma():
    """ISA audit of the cross-compiled unit; it reads the spill and private-segment metadata and the MFMA mnemonic."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = Path(__file__).resolve().parent.parent / "brainmagick_amd" / "csrc"
    with tempfile.TemporaryDirectory(prefix="bm_asm_") as tmp:
        out = Path(tmp) / "resample.s"
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{csrc}",
                        "-o", str(out), str(csrc / "resample.hip")], check=True, capture_output=True)
        text = out.read_text()
    bodies = dict(re.findall(r"^(_Z\d+\w*_kernel\w*):(.*?)^\.Lfunc_end", text, flags=re.M | re.S))
    assert len(bodies) == 2, sorted(bodies)                  # resample_mfma, resample_fma
    mfma = [k for k in bodies if "resample_mfma" in k]
    assert len(mfma) == 1 and "v_mfma_f32_16x16x4_f32" in bodies[mfma[0]]
    spills = [int(l.split(":")[1]) for l in text.splitlines() if ".vgpr_spill_count" in l or ".sgpr_spill_count" in l]
    scratch = [int(l.split(":")[1]) for l in text.splitlines() if ".private_segment_fixed_size" in l]
    assert len(spills) == 4 and len(scratch) == 2
    assert all(s == 0 for s in spills) and all(s == 0 for s in scratch), (spills, scratch)
