"""The mel spectrogram on the GPU: ``bm_wave_moments`` and ``bm_mel_spectrogram`` (csrc/mel.hip) through
``hip_ops.mel_spectrograms`` / ``wave_moments`` and ``audio.DeviceMelSpectrum``.

The truth is always the fp64 restatement on the CPU (tests/mel_cases.py: ``stft_mel`` in fp64) fed the normalised
waveform as computed here from fp64 statistics and rounded once to fp32.  Tolerance, the project's rule for fp32 against
fp64: a case's largest deviation from that truth may be at most ``TOL_FACTOR`` = 4 times the deviation of the
reference-side fp32 evaluation (``stft_mel`` in fp32, computed live) of the same input from the same truth -- of the log
output, or, without the logarithm, per frame and divided by the frame's total power.  Frames of exact zeros must be
exact.  Every figure is printed before it is asserted (``pytest -s``).

Measured on an MI355X: worst ratio 2.40 with every switch at its default (the fixture's 4000-sample waveform), 1.32
without ``norm_audio``, 1.24 without the logarithm, 1.60 without ``normalized``, 1.25 at the tile boundaries of ``n_fft``
= 512; the moments equal numpy's to the last bit at all three lengths.
"""
import math

import numpy as np
import pytest
import torch

import features_cases as FC
import mel_cases as MC
from test_segments_gpu import bits

pytestmark = pytest.mark.gpu

SR = 16_000
SWITCHES = [dict(), dict(norm_audio=False), dict(use_log_scale=False), dict(normalized=False)]     # what the fixture holds
SWITCH_IDS = ["default", "no_norm_audio", "no_log", "no_normalized"]
DEFAULTS = dict(norm_audio=True, use_log_scale=True, normalized=True, log_scale_eps=1e-5)


@pytest.fixture(scope="module")
def H():
    from brainmagick_amd import hip_ops
    return hip_ops


def make_wave(L: int, seed: int, silence=None) -> torch.Tensor:
    g = torch.Generator().manual_seed(seed)
    t = torch.arange(L) / SR
    x = 0.3 * torch.sin(2 * math.pi * 440.0 * t) + 0.2 * torch.randn(L, generator=g) + 0.05
    if silence:
        x[silence[0]:silence[1]] = 0.0
    return x.float()


def tile_lengths(H, n_fft: int):
    """One frame short of, exactly at and one frame past two of the kernel's frame tiles."""
    hop, tile = n_fft // 4, H.mel_frame_tile(n_fft)
    return [(2 * tile - 2) * hop + 1, (2 * tile - 1) * hop, 2 * tile * hop + hop - 1]


def shapes(H):
    out = [("3_frames", 16, 3, make_wave(9, 1)),
           ("ref_test_shape", 100, 8, make_wave(1000, 2)),
           ("silence_120", 512, 120, make_wave(4000, 3, (1650, 2350))),
           ("shortest", 512, 40, make_wave(257, 4))]
    for i, L in enumerate(tile_lengths(H, 16)):
        out.append((f"tiles16_{L}", 16, 3, make_wave(L, 5 + i)))
    for c in MC.fixture_cases():
        if c["name"] in ("ref_test", "silence_120", "no_norm_audio"):           # the three distinct inputs of the fixture
            out.append((f"fixture_{c['name']}", c["n_fft"], c["n_mels"], torch.mean(c["wave"], dim=0)))
    return out


_truths = {}


def truths(name, mono, n_fft, n_mels, sw):
    """(truth fp64, the reference side's own deviation), computed once per (shape, switches)."""
    key = (name, tuple(sorted(sw.items())))
    if key not in _truths:
        x = MC.normalise64(mono) if sw["norm_audio"] else mono
        truth = MC.finish(MC.stft_mel(x.double(), n_fft, n_mels, SR, sw["normalized"]), sw["use_log_scale"], sw["log_scale_eps"])
        ref32 = MC.finish(MC.stft_mel(x, n_fft, n_mels, SR, sw["normalized"]), sw["use_log_scale"], sw["log_scale_eps"])
        power = MC.stft_power(x.double(), n_fft, sw["normalized"])
        _truths[key] = (truth, MC.deviation(ref32, truth, sw["use_log_scale"]), (power == 0).all(0))
    return _truths[key]


def check_values(name, got, mono, n_fft, n_mels, sw):
    truth, ref_dev, zero_frames = truths(name, mono, n_fft, n_mels, sw)
    got = got.cpu()
    assert got.shape == truth.shape and got.dtype == torch.float32
    live = ~zero_frames
    dev = MC.deviation(got[:, live], truth[:, live], sw["use_log_scale"]) if bool(live.any()) else 0.0
    ratio = dev / ref_dev if ref_dev > 0 else (0.0 if dev == 0 else math.inf)
    print(f"mel {name} {sw}: deviation {dev:.3e}, reference side {ref_dev:.3e}, ratio {ratio:.2f}")
    if bool(zero_frames.any()):                                 # exact zeros in: exactly 0, or log10f(eps) within 4 ulp
        z = got[:, zero_frames]
        if sw["use_log_scale"]:
            want = np.float32(np.log10(np.float32(sw["log_scale_eps"])))
            assert float((z - float(want)).abs().max()) <= 4 * float(np.spacing(np.abs(want)))
        else:
            assert bool((z == 0).all())
    assert dev <= MC.TOL_FACTOR * ref_dev, (name, sw, dev, ref_dev)
    return ratio


@pytest.mark.parametrize("switch", SWITCHES, ids=SWITCH_IDS)
def test_values_against_the_fp64_restatement(H, switch):
    sw = dict(DEFAULTS, **switch)
    worst = 0.0
    for name, n_fft, n_mels, mono in shapes(H):
        got, = H.mel_spectrograms([mono.cuda()], n_mels, n_fft, SR, sw["normalized"], sw["use_log_scale"],
                                  sw["log_scale_eps"], sw["norm_audio"])
        worst = max(worst, check_values(name, got, mono, n_fft, n_mels, sw))
    print(f"mel worst ratio {switch}: {worst:.2f}")


def test_tile_boundaries_at_512(H):
    sw = dict(DEFAULTS)
    for i, L in enumerate(tile_lengths(H, 512)):
        mono = make_wave(L, 20 + i)
        got, = H.mel_spectrograms([mono.cuda()], 40, 512, SR)
        assert got.shape[1] == 1 + L // 128
        check_values(f"tiles512_{L}", got, mono, 512, 40, sw)


def test_the_silent_frames_are_there(H):
    """The silence case does hold frames of exact zeros without ``norm_audio`` and an all-zero filter row."""
    mono = make_wave(4000, 3, (1650, 2350))
    _, _, zero_frames = truths("silence_120", mono, 512, 120, dict(DEFAULTS, norm_audio=False))
    assert int(zero_frames.sum()) == 2
    _, lo, hi = H.mel_filterbank(512, 120, SR)
    got, = H.mel_spectrograms([mono.cuda()], 120, 512, SR)
    empty = (hi == lo)
    want = np.float32(np.log10(np.float32(1e-5)))
    assert bool(empty.any()) and float((got.cpu()[empty] - float(want)).abs().max()) <= 4 * float(np.spacing(np.abs(want)))


@pytest.mark.parametrize("n_fft", [16, 512])
def test_one_call_two_launches_one_order(H, n_fft):
    past = tile_lengths(H, 16)[2]
    waves = [make_wave(L, 30 + i).cuda() for i, L in enumerate((9, 257, 300, 4000, past)) if L > n_fft // 2]
    assert len(waves) == (5 if n_fft == 16 else 4)              # 9 samples are too short for n_fft = 512
    timer = H.KernelTimer()
    H.set_kernel_timer(timer)
    try:
        outs = H.mel_spectrograms(waves, 3 if n_fft == 16 else 40, n_fft, SR)
    finally:
        H.set_kernel_timer(None)
    assert [r[0] for r in timer.records] == ["wave_moments", "mel_spectrogram"]     # every launch goes through the timer
    again = H.mel_spectrograms(waves, 3 if n_fft == 16 else 40, n_fft, SR)
    moments = H.wave_moments(waves)
    storage = {o.untyped_storage().data_ptr() for o in outs}
    assert len(storage) == 1                                                       # carved from one allocation
    for i, x in enumerate(waves):
        alone, = H.mel_spectrograms([x], 3 if n_fft == 16 else 40, n_fft, SR)
        assert outs[i].shape == (3 if n_fft == 16 else 40, 1 + x.numel() // (n_fft // 4))
        assert torch.equal(bits(outs[i]), bits(alone)), i
        assert torch.equal(bits(outs[i]), bits(again[i])), i
        assert torch.equal(H.wave_moments([x]).view(torch.int64), moments[i:i + 1].view(torch.int64)), i
    timer = H.KernelTimer()
    H.set_kernel_timer(timer)
    try:
        H.mel_spectrograms(waves, 3 if n_fft == 16 else 40, n_fft, SR, norm_audio=False)
    finally:
        H.set_kernel_timer(None)
    assert [r[0] for r in timer.records] == ["mel_spectrogram"]


@pytest.mark.parametrize("L", [9, 4000, 70_001])
def test_moments_against_numpy(H, L):
    """The waveform has a mean of the size of its spread: a mean near zero would make ANY fp64 sum's relative error
    large (numpy's own included) -- the bound below is about the arithmetic, not about conditioning."""
    x = (0.3 * torch.randn(L, generator=torch.Generator().manual_seed(L)) + 0.7).float()
    assert H.lib().bm_wave_moments_splits(L) == {9: 1, 4000: 1, 70_001: 5}[L]       # several splits, a ragged last one
    mom = H.wave_moments([x.cuda()]).cpu().numpy()
    x64 = x.numpy().astype(np.float64)
    mean, std = np.mean(x64), np.std(x64, ddof=1)
    print(f"moments L={L}: mean rel {abs(mom[0, 0] - mean) / abs(mean):.2e}, "
          f"scale rel {abs(mom[0, 1] * (1e-8 + std) - 1):.2e}")
    assert abs(mom[0, 0] - mean) <= 1e-14 * abs(mean)
    assert abs(mom[0, 1] - 1.0 / (1e-8 + std)) <= 1e-14 / (1e-8 + std)


def test_moments_of_a_constant_waveform(H):
    x = torch.full((4000,), 0.75).cuda()
    mom = H.wave_moments([x]).cpu()
    assert float(mom[0, 0]) == 0.75 and abs(float(mom[0, 1]) - 1e8) <= 1e-14 * 1e8
    out, = H.mel_spectrograms([x], 40, 512, SR)
    assert bool(torch.isfinite(out).all())


def test_a_nan_sample_stays_in_its_frames(H):
    n_fft, hop, L, at = 512, 128, 4000, 1999
    mono = make_wave(L, 40)
    bad = mono.clone()
    bad[at] = float("nan")
    _, lo, hi = H.mel_filterbank(n_fft, 120, SR)
    filled = (hi > lo)
    clean, = H.mel_spectrograms([mono.cuda()], 120, n_fft, SR, norm_audio=False)
    got, = H.mel_spectrograms([bad.cuda()], 120, n_fft, SR, norm_audio=False)
    frames = torch.arange(1 + L // hop)
    covers = (frames * hop - n_fft // 2 <= at) & (at < frames * hop + n_fft // 2)       # no reflection reaches `at`
    assert int(covers.sum()) == 4
    assert torch.equal(bits(got[:, ~covers]), bits(clean[:, ~covers]))
    assert bool(torch.isnan(got.cpu()[filled][:, covers]).all())
    got, = H.mel_spectrograms([bad.cuda()], 120, n_fft, SR, norm_audio=True)
    assert bool(torch.isnan(got.cpu()[filled]).all())


def test_misaligned_waveforms_and_guarded_outputs(H):
    from test_guard_bands_gpu import Arena
    lengths = (257, 4000, tile_lengths(H, 512)[2])
    monos = [make_wave(L, 50 + i) for i, L in enumerate(lengths)]
    want = H.mel_spectrograms([m.cuda() for m in monos], 40, 512, SR)
    want_mom = H.wave_moments([m.cuda() for m in monos])
    shifted = []
    for m in monos:
        buf = torch.full((m.numel() + 8,), float("nan"), device="cuda")
        off = 1 + (-(buf.data_ptr() // 4)) % 4                  # one float past a 16-byte boundary
        view = buf[off:off + m.numel()]
        view.copy_(m)
        assert view.data_ptr() % 16 == 4
        shifted.append(view)
    arena = Arena()
    with arena.active():
        got = H.mel_spectrograms(shifted, 40, 512, SR)
        got_mom = H.wave_moments(shifted)
    arena.check("mel_spectrograms")
    assert torch.equal(got_mom.view(torch.int64), want_mom.view(torch.int64))
    for g, w in zip(got, want):
        assert not bool(torch.isnan(g).any())                   # every element of the poisoned allocation was written
        assert torch.equal(bits(g), bits(w))


def test_wiring_into_the_features_builder_and_a_train_step(H):
    from brainmagick_amd import synthetic
    from brainmagick_amd.audio import DeviceMelSpectrum
    from brainmagick_amd.features import DeviceEvents, DeviceFeaturesBuilder
    from brainmagick_amd.losses import L2Loss
    from brainmagick_amd.models import SimpleConv
    from brainmagick_amd.solver import Solver
    sr, T = 120.0, 87
    mel = DeviceMelSpectrum(sr)
    stereo = torch.stack([make_wave(8000, 60), make_wave(8000, 61)]).cuda()
    arrays = mel.compute([stereo, make_wave(6400, 62).cuda()], [SR, SR])
    assert [tuple(a.shape) for a in arrays] == [(40, 63), (40, 51)]
    one, = mel.compute([stereo], SR)
    assert torch.equal(bits(one), bits(arrays[0]))
    builder = DeviceFeaturesBuilder([mel.feature()], sr)
    host = dict(sound=dict(start=[0.1, 0.9], duration=[0.5, 0.4], MelSpectrum=[a.cpu().numpy() for a in arrays]))
    events = DeviceEvents(builder, dict(sound=dict(start=[0.1, 0.9], duration=[0.5, 0.4], MelSpectrum=arrays)))
    assert events.sources[0][0][0].data_ptr() == arrays[0].data_ptr()                  # as they are: read in place
    table = H.EventTable(builder.plan(), len(builder.kinds), builder.mask_kind, [(events.kind_tables, events.sources)], "cuda")
    firsts = [0, 60]                                                                   # the first straddles the end of event 0
    times = [FC.window_times(s, T, sr) for s in firsts]
    rec = torch.zeros(2, dtype=torch.int32, device="cuda")
    wstart = torch.tensor([t[0] for t in times], dtype=torch.float64, device="cuda")
    wdur = torch.tensor([t[1] for t in times], dtype=torch.float64, device="cuda")
    flag = torch.zeros(1, dtype=torch.int32, device="cuda")
    feats, mask = H.segment_features(table, rec, wstart, wdur, 0, 2, T, sr, flag)
    specs = [FC.feature("MelSpectrum", "resampled", "sound", 40, default_value=mel.default_value)]
    want = np.stack([FC.build_window(specs, False, host, *t, sr, T)[0] for t in times])
    assert torch.equal(bits(feats), bits(torch.from_numpy(want))) and int(flag.item()) == 0
    gap = feats[0, :, 75:]                                                             # 0.6 s ... 0.725 s: no sound
    assert bool((gap == np.float32(mel.default_value)).all()) and bool((feats[0, :, 20:60] != np.float32(-5.0)).any())
    batch = synthetic.make_batch(2, 8, T, 40, 2, seed=7)
    batch.features, batch.features_mask = feats, mask
    torch.manual_seed(0)
    model = SimpleConv(in_channels={"meg": 8}, out_channels=40, hidden={"meg": 16}, n_subjects=2, depth=2, kernel_size=3,
                       merger=False, subject_layers=False, subject_dim=0)
    loss = Solver(model, loss=L2Loss()).train_step(batch.to("cuda"))
    assert bool(torch.isfinite(loss))
