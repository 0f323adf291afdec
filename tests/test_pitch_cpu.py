"""The host side of the Pitch feature without a GPU: the direct-form restatement of YIN (tests/audio_cases.py) against
the fixture of the live reference (tests/golden/make_audio_rates_golden.py), the attributes of ``DevicePitch``, every
limit, the declared entry points and the ISA of csrc/pitch.hip.  Reads the fixture only."""
import inspect
import re
import shutil
import subprocess
import tempfile
from pathlib import Path

import numpy as np
import pytest
import torch

import audio_cases as AC

FX = AC.fixture()
PITCH_CASES = [(c["params"], c["signal"]) for c in FX["meta"]["pitch"]]


def test_the_fixture_holds_what_the_issue_asks_for():
    assert set(PITCH_CASES) == {("default", s) for s in ("voiced", "mixed", "len_w1", "len_ws", "len_ws1")} | \
        {("wide", "voiced"), ("wide", "mixed")}
    assert FX["meta"]["smallest_margin"] >= 1e-9                 # no comparison of any frame is a near tie
    assert FX["meta"]["frames"] > 500 and FX["meta"]["voiced"] > 300
    for name, sig in AC.pitch_signals().items():                 # the signals are seeded: the fixture holds the same
        assert np.array_equal(sig.numpy(), FX[f"signal/{name}"]), name
    assert np.array_equal(AC.stereo_441().numpy(), FX["wiring/wave"])


@pytest.mark.parametrize("params,signal", PITCH_CASES)
def test_direct_form_equals_the_fixture(params, signal):
    kw = AC.yin_kwargs(AC.PITCH_PARAMS[params])
    sig = FX[f"signal/{signal}"]
    got, margin = AC.yin_direct(sig, 16_000, **kw)
    want = FX[f"pitch/{params}/{signal}"]
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape == (len(range(0, len(sig) - kw["w_len"],
                                                                                                   kw["w_step"])),)
    assert np.array_equal(got, want)
    assert margin >= 1e-9


def test_frame_counts_at_the_boundary_lengths():
    from brainmagick_amd import hip_ops as H
    assert [FX[f"pitch/default/{s}"].shape[0] for s in ("len_w1", "len_ws", "len_ws1")] == [1, 1, 2]
    assert [H.yin_frames(L, 256, 64) for L in (257, 320, 321, 16_000)] == [1, 1, 2, 246]


def test_silent_noise_and_voiced_stretches():
    want = FX["pitch/default/mixed"]
    starts = np.arange(len(want)) * 64
    silent = (starts >= 4000) & (starts + 256 <= 7000)
    noise = (starts >= 10_000) & (starts + 256 <= 13_000)
    assert silent.sum() > 30 and bool((want[silent] == 0).all())             # 0 / 0: every comparison is false
    assert bool((want[noise] == 0).mean() > 0.9)
    voiced = FX["pitch/default/voiced"]
    assert bool(((voiced > 135) & (voiced < 225)).mean() > 0.95)             # the vibrato between 140 and 220 Hz


def test_the_wiring_case_resamples_before_yin():
    """``Pitch._compute``: channel mean -> resampler -> YIN, no normalisation; the fp64 record equals the restated chain
    exactly (its comparisons keep a margin of 1e-9), the fp32 record has the same length."""
    stereo = torch.from_numpy(FX["wiring/wave"])
    kw = AC.yin_kwargs(AC.PITCH_PARAMS["default"])
    at16 = AC.ResampleFrac(44_100, 16_000)(torch.mean(stereo.double(), dim=0))
    assert at16.numel() == 16_000 * stereo.shape[1] // 44_100 == 4000
    got, margin = AC.yin_direct(at16.numpy(), 16_000, **kw)
    assert margin >= 1e-9 and np.array_equal(got, FX["wiring/pitch/out64"])
    assert FX["wiring/pitch/out32"].shape == got.shape == (59,)
    assert float(np.abs(FX["wiring/pitch/out32"] - got).max()) <= 1e-3 * float(got.max())
    assert bool((got > 0).mean() > 0.8)


def test_device_pitch_attributes_and_defaults():
    from brainmagick_amd.audio import DevicePitch
    sig = inspect.signature(DevicePitch)
    got = {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty}
    assert got == AC.PITCH_PARAMS["default"]
    feature = DevicePitch(120.0)
    assert (feature.in_sampling, feature.dimension, feature.event_kind, feature.default_value) == (16_000, 1, "sound", 0.0)
    assert feature.sample_rate == 120.0
    for k, v in AC.PITCH_PARAMS["default"].items():
        assert getattr(feature, k) == v
    ef = feature.feature()
    assert (ef.name, ef.rule, ef.event_kind, ef.dimension, ef.default_value) == ("Pitch", "resampled", "sound", 1, 0.0)
    assert DevicePitch(120.0, **AC.PITCH_PARAMS["wide"]).frame_length_in_samples == 512


def test_every_limit_raises_its_value_error():
    from brainmagick_amd import hip_ops as H
    from brainmagick_amd.audio import DevicePitch
    wave = torch.zeros(4000)
    with pytest.raises(ValueError, match="L > w_len"):
        H.yin_pitch([torch.zeros(256)])
    with pytest.raises(ValueError, match="tau_max"):
        H.yin_pitch([wave], f0_min=50.0)                                     # 320 > w_len = 256
    with pytest.raises(ValueError, match="tau_min"):
        H.yin_pitch([wave], f0_max=20_000.0)
    with pytest.raises(ValueError, match="w_len"):
        H.yin_pitch([wave], w_len=2048)
    with pytest.raises(ValueError, match="w_step"):
        H.yin_pitch([wave], w_step=1024)
    with pytest.raises(ValueError, match="w_step"):
        H.yin_pitch([wave], w_step=0)
    with pytest.raises(ValueError, match="positive"):
        H.yin_pitch([wave], f0_min=0.0)
    with pytest.raises(ValueError, match=r"2\^31"):
        H.yin_pitch([torch.empty(2 ** 31, device="meta")])
    with pytest.raises(ValueError, match="limit is 65535"):
        H.yin_pitch([wave] * 65536)
    with pytest.raises(ValueError, match="tau_max"):
        DevicePitch(120.0, min_f0=50.0)
    with pytest.raises(ValueError, match="w_len"):
        DevicePitch(120.0, frame_length_in_samples=4096)
    with pytest.raises(RuntimeError):                                        # within the limits: no CPU fallback
        H.yin_pitch([wave])
    with pytest.raises(RuntimeError):
        DevicePitch(120.0).compute([wave], 16_000)
    assert H.yin_taus(16_000, 256, 64, 100.0, 350.0) == (45, 160) and H.yin_taus(16_000, 512, 256, 100.0, 500.0) == (32, 160)


def test_library_declares_the_pitch_entry_points():
    from brainmagick_amd import _lib
    from brainmagick_amd import hip_ops as H
    L = _lib.lib()
    assert L.bm_version() >= 115 and L.bm_yin_frames_tile() == 4
    protos = _lib.parse_header()
    assert {"bm_yin_pitch", "bm_yin_frames_tile"} <= set(protos)
    assert protos["bm_yin_pitch"][2] == ["table", "lengths", "n_waves", "sr", "w_len", "w_step", "tau_min", "tau_max",
                                         "thresh", "stream"]
    sig = inspect.signature(H.yin_pitch)
    assert {k: p.default for k, p in sig.parameters.items() if p.default is not inspect.Parameter.empty} == \
        dict(sr=16_000, w_len=256, w_step=64, harmo_thresh=0.1, f0_min=100.0, f0_max=350.0)


def test_pitch_kernel_uses_no_scratch():
    """ISA audit of the cross-compiled unit; it reads the spill and private-segment metadata only."""
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    if not Path(hipcc).exists():
        pytest.skip("hipcc not available")
    csrc = Path(__file__).resolve().parent.parent / "brainmagick_amd" / "csrc"
    with tempfile.TemporaryDirectory(prefix="bm_asm_") as tmp:
        out = Path(tmp) / "pitch.s"
        subprocess.run([hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{csrc}",
                        "-o", str(out), str(csrc / "pitch.hip")], check=True, capture_output=True)
        text = out.read_text()
    bodies = dict(re.findall(r"^(_Z\d+\w*_kernel\w*):(.*?)^\.Lfunc_end", text, flags=re.M | re.S))
    assert len(bodies) == 1 and "yin_pitch" in next(iter(bodies)), sorted(bodies)
    spills = [int(l.split(":")[1]) for l in text.splitlines() if ".vgpr_spill_count" in l or ".sgpr_spill_count" in l]
    scratch = [int(l.split(":")[1]) for l in text.splitlines() if ".private_segment_fixed_size" in l]
    assert len(spills) == 2 and len(scratch) == 1
    assert all(s == 0 for s in spills) and all(s == 0 for s in scratch), (spills, scratch)
